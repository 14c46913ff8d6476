/*
 * subdomain.hpp -- Subdomain<DType>: the full-domain-decomposition
 * preconditioner host class of the reference (subdomain.hpp:72-252), solve
 * path only (subdomain.tpp:3942-4646): tree_operator, stiffness_matrix,
 * direct_stiffness_summation, the inner flexible GMRES(4) and flexible CG and
 * their local reductions -- no communication inside the inner solve, which is
 * the FDD property.
 *
 * THE COMPOSITE.  The reference's constructor (subdomain.tpp:86-3705) builds a
 * composite of: own elements at degree N, rings of neighbour elements at
 * reduced degree, and an algebraically coarsened superdomain.  With more than
 * one rank that composite is built by composite.hpp (regions, ring-data pull,
 * non-conforming Q with J_cf rows, superdomain A / Pt, interface maps, weights)
 * and this class runs the reference's solve path on it: tree_operator with its
 * exchange half (ring pull by grouped send / receive, coarse level by
 * all-gather, Qt_coarse, Pt), mixed-degree stiffness on level-sorted element
 * lists plus the CSR tail, the Q / QQt_int / Qt chain, weighted norms.  The one
 * labelled deviation: the superdomain is graded by this build's own smoothed
 * aggregation where the reference walks HYPRE BoomerAMG's hierarchy
 * (composite.hpp).  `block_local = true` keeps the rank's own elements only
 * (no rings, no superdomain: block-Jacobi, kept as the comparison point).
 *
 * With one rank the region holds the rank's own conforming elements and the
 * constructor reduces to:
 *   - dof_num = dense rank of glo_num*mask, 0 on Dirichlet points
 *     (ranking lambda subdomain.tpp:881-918, applied at :1151-1176);
 *   - Q one 1.0 per non-Dirichlet point (subdomain.tpp:1517-1520), Qt = Q^T;
 *   - Q_int = Qt_int = QQt_int = I (subdomain.tpp:2653-2729 with no
 *     interface / extended dofs), norm_weight = 1, inner_weight = (Q*1 > 0)
 *     (subdomain.tpp:2731-2747);
 *   - superdomain_operator.A / .Pt empty: their multiplies are the no-ops of
 *     csr_matrix.tpp:304, 334.
 *
 * MI355X-first changes underneath: the mixed-degree element kernels run
 * level-sorted (one fused launch per polynomial level over that level's
 * element list) instead of reading offset/vertex/level per point
 * (subdomain.okl:10-15); the three restriction launches per level pair are one
 * LDS-staged launch; dot products finish on the device.
 */
#ifndef FDD_SUBDOMAIN_HPP
#define FDD_SUBDOMAIN_HPP

#include <algorithm>
#include <cmath>
#include <map>
#include <stdexcept>
#include <unordered_map>
#include <chrono>
#include <vector>

#include "amg.hpp"
#include "amg_device_setup.hpp"
#include "assembly_classes.hpp"
#include "composite.hpp"
#include "config.hpp"
#include "csr_matrix.hpp"
#include "domain.hpp"
#include "element_operator.hpp"
#include "fdd_norm_estimate.h"
#include "gll.hpp"
#include "gmres.hpp"
#include "low_order.hpp"
#include "math.hpp"
#include "timer.hpp"

template <typename DType>
struct Stiffness_Operator // subdomain.hpp:46-70
{
    int num_dofs = 0;
    int num_points = 0;
    int num_extended_dofs = 0;

    CSR_Matrix<DType> Q;
    CSR_Matrix<DType> Qt;

    CSR_Matrix<DType> A;
    CSR_Matrix<DType> P;
    CSR_Matrix<DType> Pt;

    fdd::memory geom_fact[NUM_GEOM_FACTS];

    std::vector<fdd::LevelList> level_lists; // one per polynomial level present (element_operator.hpp)
};

template <typename DType>
class Subdomain
{
  private:
    std::vector<fdd::memory> work_dev;

    int poly_reduction = 1;
    int subdomain_overlap = 1;
    int superdomain_overlap = 1;

    std::vector<int> poly_degree;
    int num_levels = 0;

    struct Level // subdomain.hpp:89-95
    {
        int num_points;
        int num_elements;
        int poly_degree;
        int offset;
    };
    std::vector<Level> levels;

    // coarse-to-fine interpolators, key (N_c, N_f) (subdomain.hpp:100)
    std::map<std::pair<int, int>, std::pair<std::vector<DType>, fdd::memory>> J_cf;

    std::vector<std::pair<std::vector<DType>, fdd::memory>> D_hat;

    Stiffness_Operator<DType> subdomain_operator;
    Stiffness_Operator<DType> superdomain_operator;
    CSR_Matrix<DType> Qt_coarse;

    int num_interface_dofs = 0;
    CSR_Matrix<DType> Q_int, Qt_int, QQt_int;

    int num_dofs = 0;
    int num_blocks = 0;
    fdd::memory norm_weight;
    fdd::memory inner_weight;

    fdd::memory f, u_k, r_k, r_kp1, q_k, z_k, p_k;
    std::vector<fdd::memory> V, Z;
    fdd::GmresScalars<DType> gmres_scalars; // H, rotations, gamma of the host-bookkeeping inner GMRES, sized per solve

    fdd::memory reduce_ws;
    fdd::memory scalars;

    // the dof-space vectors of the inner solve, one set per precision of the preconditioner
    template <typename Real>
    struct DofKrylov
    {
        std::vector<fdd::memory> VA; // assembled (dof-space) copies Qt_w V[i] of the Krylov basis
        fdd::memory qa;              // Qt_w q
        std::vector<fdd::memory> ZA; // preconditioned basis (only with the V-cycle or point-Jacobi in the slot)
        fdd::memory ua, fa;          // solution and right-hand side over the dofs (allocated by the solves that do not work on the caller's)
        // m + 1 basis vectors and qa of na entries, and with keep_Z the m preconditioned ones: storage made for another
        // num_vectors is replaced
        void ensure(int m, int na, bool keep_Z)
        {
            if ((int)VA.size() != m + 1)
            {
                VA.resize(m + 1);
                for (auto &v : VA) v = fdd::dev().malloc<Real>(na);
                qa = fdd::dev().malloc<Real>(na);
            }
            if (keep_Z and (int)ZA.size() != m)
            {
                ZA.resize(m);
                for (auto &v : ZA) v = fdd::dev().malloc<Real>(na);
            }
        }
    };
    DofKrylov<double> krylov64;
    DofKrylov<float> krylov32;
    fdd::memory point_dof_dev;   // dof of every level-0 point (-1: none): Q as an index array
    fdd::memory gmres_state;     // device-side GMRES bookkeeping (fdd_gmres_*_dev)
    bool norm_weight_is_one = false; // norm_weight == 1 everywhere (subdomain.tpp:2731-2747 without interface dofs)
    const MeshData<DType> *fine_mesh = nullptr; // level-0 coordinates (low-order FEM assembly)

    fdd::memory points_without_dof; // Dirichlet points: empty rows of Q
    int num_points_without_dof = 0;

    // ---- composite region (more than one rank): composite.hpp builds it, this class runs on it ----
    bool is_composite = false;
    fdd::composite::Composite comp;            // host description; the big per-point arrays are released after the upload
    int own_points = 0;                        // points of the rank's own elements = head of every composite vector
    fdd::memory ring_geom[NUM_GEOM_FACTS];     // geometric factors of the whole region when it has ring elements (own elements copied in: one list per degree)
    std::vector<DType> norm_weight_hst;
    // tree exchange (subdomain.tpp:4615-4644), all on device buffers
    fdd::memory send_index, send_all, recv_all, unpack_index; // pack: send_all[k] = tree[send_index[k]]; unpack: head ring part [i] = recv_all[unpack_index[i]]
    std::vector<fdd::ExchangeOp> exchange_ops;
    // The coarse level's all-gather folded into the ring pull's group: every rank sends its degree-1 block straight to every
    // other rank in the same grouped send / receive (xGMI gives every pair of GPUs its own link: 7 direct messages of one
    // block each instead of a ring all-gather that carries 7 blocks over every link, and one group instead of two
    // collectives per preconditioner application).  Same bytes in the same places; fold_coarse_exchange = false keeps
    // the all-gather (subdomain.tpp:4620-4621).
    std::vector<fdd::ExchangeOp> exchange_ops_folded;
    int num_send_points = 0, num_ring_points = 0;
    fdd::memory coarse_all;                    // the all-gathered degree-1 level of every rank, `coarse_pad` values per rank
    int coarse_pad = 0;
    // dof-space form of the composite (see setup_composite_dofs)
    bool comp_dofs_ready = false;
    int n_sup_copies = 0, n_slaves = 0, slave_base = 0, W_len = 0;
    fdd::memory copy_src;                      // int[n_sup_copies]: the subdomain dof every superdomain-extended dof copies
    CSR_Matrix<DType> S_slave, St_slave;       // hanging points: their J_cf rows over the subdomain dofs, and the transpose's NON-EMPTY rows
    fdd::memory st_rows, st_tmp;               //   (a few thousand of millions of dofs): the dof of each such row, and its product
    CSR_Matrix<DType> G_ring;                  // own dofs that ring points also feed: those points, by compressed rows (right-hand side from the node residual)
    fdd::memory ring_rows, ring_tmp;
    CSR_Matrix<DType> G_unit;                  // boolean gather: rows = subdomain dofs then hanging points, columns = region points
    CSR_Matrix<DType> A_sup_reg;               // rows of the superdomain operator that belong to its regular dofs
    fdd::memory slave_vals;                    // gathered values of the hanging points

    Math<DType> math;
    int dim = 3;

    // ranking lambda of the reference (subdomain.tpp:881-918): dense ranks, 0 stays 0
    static void ranking(std::vector<double> &data)
    {
        const size_t size = data.size();
        if (size == 0) return;
        std::vector<std::pair<double, unsigned int>> entries(size);
        for (size_t i = 0; i < size; i++) entries[i] = std::make_pair(data[i], (unsigned int)i);
        std::sort(entries.begin(), entries.end());
        double value = entries[0].first;
        double rank = (value == 0.0) ? 0.0 : 1.0;
        data[entries[0].second] = rank;
        for (size_t i = 1; i < size; i++)
        {
            if (entries[i].first != value)
            {
                rank += 1.0;
                value = entries[i].first;
            }
            data[entries[i].second] = rank;
        }
    }

    static void identity_matrix(CSR_Matrix<DType> &A, int n) { A.initialize_identity(n); }

    void fetch_scalars(DType *out, int n) { scalars.copyTo(out, n * sizeof(DType)); }

    void initialize_arrays(fdd::memory &u, fdd::memory &r, fdd::memory &ff) // subdomain.tpp:4270-4275
    {
        FDD_CALL(fdd_sub_initialize_arrays(u.as<double>(), r.as<double>(), ff.as<double>(), num_values, fdd::dev().stream));
    }

    // subdomain.tpp:4566-4646
    void tree_operator(fdd::memory &Tu, fdd::memory &u)
    {
        // Level 0 of the tree is the caller's vector (copy_from_domain_data, subdomain.tpp:4571).  The composite reads it
        // where it lies (first restriction, ring packing, own part of the result); the other paths keep the copy.
        fdd_timer().start("subdomain.tree_construction.gpu_to_gpu");
        if (not is_composite) FDD_CALL(fdd_sub_copy_f64_f64(work_dev[0].as<double>(), u.as<double>(), levels[0].num_points, fdd::dev().stream));
        fdd_timer().stop("subdomain.tree_construction.gpu_to_gpu");

        fdd_timer().start("subdomain.tree_construction.subdomain");
        if (build_tree or is_composite) // the composite's rings and superdomain are fed by the tree
        {
            for (int l = 0; l < num_levels - 1; l++)
            {
                const int n_f = levels[l].poly_degree + 1;
                const int n_c = levels[l + 1].poly_degree + 1;
                fdd::memory &J = J_cf[std::pair<int, int>(levels[l + 1].poly_degree, levels[l].poly_degree)].second;
                fdd::memory u_f = (l == 0 and is_composite) ? u.slice(0, levels[0].num_points) : work_dev[0].slice(levels[l].offset, levels[l].num_points);
                fdd::memory u_c = work_dev[0].slice(levels[l + 1].offset, levels[l + 1].num_points);

                if (dim == 3)
                {
                    fdd::ProfileScope prof("restriction_fused_kernel", 8.0 * levels[l].num_elements * ((double)n_f * n_f * n_f + (double)n_c * n_c * n_c));
                    FDD_CALL(fdd_sub_restriction(u_c.as<double>(), J.as<double>(), u_f.as<double>(), levels[l].num_elements, n_f, n_c, fdd::dev().stream));
                }
                else
                {
                    // the two `dim == 2` launches (subdomain.tpp:4593-4596) as one, bit-identical
                    fdd::ProfileScope prof("restriction_2d_kernel", 8.0 * levels[l].num_elements * ((double)n_f * n_f + (double)n_c * n_c));
                    FDD_CALL(fdd_sub_restriction_2d(u_c.as<double>(), J.as<double>(), u_f.as<double>(), levels[l].num_elements, n_f, n_c, fdd::dev().stream));
                }
            }
        }
        fdd_timer().stop("subdomain.tree_construction.subdomain");

        if (is_composite)
        {
            tree_exchange(Tu, u);
            return;
        }

        // Tree exchange.  With only own elements in the region the gs pull of
        // subdomain.tpp:4626-4630 is a device copy of the level-0 slice; the
        // coarse level has no superdomain consumer, so no all-gather is issued.
        fdd_timer().start("subdomain.tree_exchange.subdomain");
        Tu.copyFrom(work_dev[0], (size_t)subdomain_operator.num_points * sizeof(DType));
        fdd_timer().stop("subdomain.tree_exchange.subdomain");

        if (build_tree and Qt_coarse.num_rows > 0)
        {
            fdd_timer().start("subdomain.tree_construction.assemble_coarse");
            fdd::memory coarse = work_dev[0].slice(levels[num_levels - 1].offset, levels[num_levels - 1].num_points);
            Qt_coarse.multiply(work_dev[1], coarse); // subdomain.tpp:4639
            fdd_timer().stop("subdomain.tree_construction.assemble_coarse");
        }
        // superdomain_operator.Pt.multiply: empty matrix (subdomain.tpp:4643-4644)
    }

    // The exchange half of tree_operator (subdomain.tpp:4613-4645), on device buffers throughout where the
    // reference stages the whole tree through the host:
    //   ring pull     gslib gs on (+owner, -copy) ids (:4626)  ->  pack, ONE grouped send / receive with the ranks
    //                 whose regions overlap this one, unpack into the ring part of the head;
    //   coarse level  MPI_Allgatherv (:4620-4621)               ->  all-gather (fixed count per rank, Qt_coarse
    //                 addresses the padded layout), then Qt_coarse and Pt into the tail (:4639-4644).
    void tree_exchange(fdd::memory &Tu, fdd::memory &u)
    {
        void *stream = fdd::dev().stream;
        fdd_timer().start("subdomain.tree_exchange.subdomain");
        // level 0 of the tree is `u` itself, the restricted levels are in work_dev[0] at their tree offsets
        if (num_send_points > 0) FDD_CALL(fdd_gather_indexed_split(send_all.as<double>(), u.as<double>(), work_dev[0].as<double>(), levels[0].num_points, send_index.template as<int>(), num_send_points, stream));
        const bool coarse_needed = fdd::comm().size > 1 or superdomain_operator.num_extended_dofs > 0; // rank-uniform (see below)
        const bool folded = fold_coarse_exchange and fdd::comm().size > 1;
        fdd::memory coarse = work_dev[0].slice(levels[num_levels - 1].offset, coarse_pad);
        if (folded)
        {
            // own block in place, the others by the group below
            FDD_CALL(fdd_memcpy_d2d(coarse_all.as<DType>() + (size_t)fdd::comm().rank * coarse_pad, coarse.ptr(), (size_t)coarse_pad * sizeof(DType), stream));
            fdd::comm().exchange(exchange_ops_folded.data(), (int)exchange_ops_folded.size());
        }
        else
            fdd::comm().exchange(exchange_ops.data(), (int)exchange_ops.size()); // every rank calls it (a rank without peers passes none): one back-end meets world-wide
        // the rank's own elements: the level-0 slice (:4630); nothing to do when the caller keeps its vector in place (tree_points())
        if (Tu.ptr() != u.ptr()) Tu.copyFrom(u, (size_t)own_points * sizeof(DType));
        if (num_ring_points > 0) FDD_CALL(fdd_gather_indexed(Tu.as<double>() + own_points, recv_all.as<double>(), unpack_index.template as<int>(), nullptr, num_ring_points, stream));
        fdd_timer().stop("subdomain.tree_exchange.subdomain");

        // The all-gather is issued by EVERY rank, as the reference's MPI_Allgatherv is (subdomain.tpp:4620): whether a
        // rank has a superdomain of its own is a per-rank fact (a rank whose rings already cover the whole domain has
        // none while its peers do), and a collective gated on it would leave the peers waiting.  Only the local
        // products below are skipped by such a rank.
        fdd_timer().start("subdomain.tree_exchange.superdomain");
        if (coarse_needed and not folded) fdd::comm().allgather(coarse.ptr(), coarse_all.ptr(), (size_t)coarse_pad * sizeof(DType));
        fdd_timer().stop("subdomain.tree_exchange.superdomain");
        if (superdomain_operator.num_extended_dofs == 0) return;

        fdd_timer().start("subdomain.tree_construction.assemble_coarse");
        Qt_coarse.multiply(work_dev[1], coarse_all); // :4639
        fdd_timer().stop("subdomain.tree_construction.assemble_coarse");

        fdd_timer().start("subdomain.tree_construction.superdomain");
        fdd::memory Tu_sup = Tu.slice(subdomain_operator.num_points, superdomain_operator.num_extended_dofs);
        superdomain_operator.Pt.multiply(Tu_sup, work_dev[1]); // :4643-4644
        fdd_timer().stop("subdomain.tree_construction.superdomain");
    }

    // subdomain.tpp:4491-4515
    void residual_norm(DType &r_norm, fdd::memory &r)
    {
        fdd::memory r_sub_l = r.slice(0, subdomain_operator.num_points);
        fdd::memory work_sub = work_dev[1].slice(0, subdomain_operator.num_extended_dofs);

        subdomain_operator.Qt.multiply_weight(work_sub, r_sub_l, norm_weight);
        copy_tail(work_dev[1], r); // r_sup.copyTo(work_sup), :4501

        const int nv = subdomain_operator.num_extended_dofs + superdomain_operator.num_extended_dofs;
        FDD_CALL(fdd_sub_weighted_inner_product(scalars.as<double>(), reduce_ws.as<double>(), work_dev[1].as<double>(), work_dev[1].as<double>(), norm_weight.as<double>(), nv, fdd::dev().stream));
        fetch_scalars(&r_norm, 1);
        r_norm = std::sqrt(r_norm);
    }

    // the superdomain part of a composite vector next to the assembled subdomain part: [ext sub dofs | ext sup dofs]
    void copy_tail(fdd::memory &dofs, fdd::memory &values)
    {
        const int nue = superdomain_operator.num_extended_dofs;
        if (nue == 0) return;
        fdd::memory dst = dofs.slice(subdomain_operator.num_extended_dofs, nue);
        dst.copyFrom(values.slice(subdomain_operator.num_points, nue), (size_t)nue * sizeof(DType));
    }
    void copy_tail_back(fdd::memory &values, fdd::memory &dofs)
    {
        const int nue = superdomain_operator.num_extended_dofs;
        if (nue == 0) return;
        fdd::memory dst = values.slice(subdomain_operator.num_points, nue);
        dst.copyFrom(dofs.slice(subdomain_operator.num_extended_dofs, nue), (size_t)nue * sizeof(DType));
    }

    // subdomain.tpp:4277-4307
    void assembled_inner_product(DType &uv, fdd::memory &u, fdd::memory &v)
    {
        fdd::memory u_sub_l = u.slice(0, subdomain_operator.num_points);
        fdd::memory u_work_sub = work_dev[0].slice(0, subdomain_operator.num_extended_dofs);
        subdomain_operator.Qt.multiply_weight(u_work_sub, u_sub_l, norm_weight);
        copy_tail(work_dev[0], u); // :4286

        fdd::memory v_sub_l = v.slice(0, subdomain_operator.num_points);
        fdd::memory v_work_sub = work_dev[1].slice(0, subdomain_operator.num_extended_dofs);
        subdomain_operator.Qt.multiply_weight(v_work_sub, v_sub_l, norm_weight);
        copy_tail(work_dev[1], v); // :4294

        const int nv = subdomain_operator.num_extended_dofs + superdomain_operator.num_extended_dofs;
        FDD_CALL(fdd_sub_weighted_inner_product(scalars.as<double>(), reduce_ws.as<double>(), work_dev[0].as<double>(), work_dev[1].as<double>(), norm_weight.as<double>(), nv, fdd::dev().stream));
        fetch_scalars(&uv, 1);
    }

    void projection_inner_products(DType &gamma_k, DType &theta_k, fdd::memory &z, fdd::memory &r, fdd::memory &p, fdd::memory &q) // :4517-4535
    {
        DType v[2];
        FDD_CALL(fdd_sub_projection_inner_products(scalars.as<double>(), reduce_ws.as<double>(), z.as<double>(), r.as<double>(), p.as<double>(), q.as<double>(), inner_weight.as<double>(), num_values, fdd::dev().stream));
        fetch_scalars(v, 2);
        gamma_k = v[0];
        theta_k = v[1];
    }

    void solution_and_residual_update(fdd::memory &u, fdd::memory &r1, fdd::memory &r, fdd::memory &p, fdd::memory &q, DType alpha_k) // :4537-4542
    {
        FDD_CALL(fdd_sub_solution_and_residual_update(u.as<double>(), r1.as<double>(), r.as<double>(), p.as<double>(), q.as<double>(), alpha_k, num_values, fdd::dev().stream));
    }

    void search_update_inner_product(DType &theta_k, fdd::memory &r, fdd::memory &r1, fdd::memory &z) // :4544-4557
    {
        FDD_CALL(fdd_sub_search_update_inner_product(scalars.as<double>(), reduce_ws.as<double>(), r.as<double>(), r1.as<double>(), z.as<double>(), inner_weight.as<double>(), num_values, fdd::dev().stream));
        fetch_scalars(&theta_k, 1);
    }

    void residual_and_search_update(fdd::memory &p, fdd::memory &r, fdd::memory &z, fdd::memory &r1, DType beta_k) // :4559-4564
    {
        FDD_CALL(fdd_sub_residual_and_search_update(p.as<double>(), r.as<double>(), z.as<double>(), r1.as<double>(), beta_k, num_values, fdd::dev().stream));
    }

    // The V-cycle's hierarchy: handed in (amg_add_level / amg_finalize), built by the caller (amg_build), or -- the
    // reference's constructor does it unconditionally, subdomain.tpp:2752 -- built here on first use with the
    // default options.  A region it cannot be built for (2-D, degree 1 without a composite) is an error, not a
    // silent identity.
    amg::Level &amg_checked()
    {
        if (not amg_hierarchy.ready() and amg_hierarchy.levels.empty() and dim == 3 and fine_mesh != nullptr and (poly_degree[0] >= 2 or is_composite))
        {
            rstdout("Assembling subdomain low-order preconditioner\n"); // subdomain.tpp:2750
            amg_build(fdd::low_order::Options());
        }
        if (not amg_hierarchy.ready() or amg_hierarchy.fine_size() != num_dofs)
        {
            fprintf(stderr, "ERROR: Subdomain::use_preconditioner = true needs an AMG hierarchy over the %d dofs (amg_add_level / amg_finalize, or amg_build: 3-D regions of degree >= 2)\n", num_dofs);
            exit(EXIT_FAILURE);
        }
        return amg_hierarchy.levels[0];
    }

    // subdomain.tpp:3987-4159: z = Q Q_int V(Qt_int Qt r), V = the AMG V-cycle on
    // the low-order FEM matrix.  The hierarchy comes from HYPRE in the reference
    // (subdomain.tpp:2749-3705) and is attached from outside here (amg.hpp);
    // asking for the preconditioner without one is an error, not a silent identity.
    void low_order_preconditioner(fdd::memory &z, fdd::memory &r)
    {
        amg::Level &fine = amg_checked();
        // this entry gives and takes double vectors; the float inner solve may have left the cycle reading f32 and writing u32
        if (amg_hierarchy.f32_io) amg_hierarchy.set_f32_io(false);
        fdd::memory r_sub_l = r.slice(0, subdomain_operator.num_points);
        fdd::memory z_sub_l = z.slice(0, subdomain_operator.num_points);
        subdomain_operator.Qt.multiply(work_dev[0], r_sub_l); // :3996
        copy_tail(work_dev[0], r);                            // :4000
        if (Qt_int.is_identity)
            fine.f.copyFrom(work_dev[0], (size_t)num_dofs * sizeof(DType)); // :4004-4008 with Qt_int = I
        else
        {
            Qt_int.multiply(work_dev[1], work_dev[0]);
            fine.f.copyFrom(work_dev[1], (size_t)num_dofs * sizeof(DType));
        }
        amg_hierarchy.vcycle(); // :4012-4142
        if (Q_int.is_identity)
            subdomain_operator.Q.multiply(z_sub_l, fine.u); // :4146-4153 with Q_int = I
        else
        {
            Q_int.multiply(work_dev[0], fine.u);
            subdomain_operator.Q.multiply(z_sub_l, work_dev[0]);
            copy_tail_back(z, work_dev[0]); // :4157
        }
    }


    // ------------------------------------------------------------------
    // POINT-JACOBI in the inner solver's preconditioner slot -- a LABELLED OPTION of this build, not in the reference,
    // whose slot holds the AMG V-cycle (use_preconditioner = true, subdomain.tpp:4373-4378) or the identity (dssum,
    // :4379-4382).  z = Q Q_int D^-1 (Qt_int Qt r) with D = diag of the operator of the inner iteration over the
    // unique dofs, (Qt A_L Q | A_sup).  Why: with the V-cycle off, four Krylov steps act on an operator whose rows
    // are scaled very differently -- GLL clustering inside an element (diagonal 0.02 ... 0.8 at N = 7), and in the
    // composite the coarse dofs that reduced-degree ring elements hang on (diagonal up to 6x the largest own row);
    // unscaled, GMRES(4) spends its four steps on those few rows (tools/composite_operator_analysis.py).
    // The diagonal is exact: sum of the element diagonals over a dof's points, and w^T A_e w for a dof that several
    // points of one element interpolate from (hanging faces / edges, the J_cf rows of Q).
    // ------------------------------------------------------------------
    fdd::memory jacobi_dinv, jacobi_dinv_f32;
    std::vector<double> jacobi_diag_hst; // the diagonal itself over the unique dofs (test hook)

    // diagonal of the element operator D^T G D (domain.okl:5-98 / subdomain.okl:4-101): the coefficient of u(i,j,k) in Au(i,j,k)
    static void element_diagonal(double *a, const std::vector<DType> &D, const double *const G[NUM_GEOM_FACTS], int n, int dim)
    {
        if (dim == 2)
        {
            for (int j = 0; j < n; j++)
                for (int i = 0; i < n; i++)
                {
                    double v = 0.0;
                    for (int p = 0; p < n; p++) v += D[i + p * n] * D[i + p * n] * G[0][p + j * n] + D[j + p * n] * D[j + p * n] * G[1][i + p * n];
                    v += 2.0 * D[i + i * n] * D[j + j * n] * G[2][i + j * n];
                    a[i + j * n] = v;
                }
            return;
        }
        const int nn = n * n;
        for (int k = 0; k < n; k++)
            for (int j = 0; j < n; j++)
                for (int i = 0; i < n; i++)
                {
                    const int v0 = i + j * n + k * nn;
                    double v = 0.0;
                    for (int p = 0; p < n; p++)
                        v += D[i + p * n] * D[i + p * n] * G[0][p + j * n + k * nn] + D[j + p * n] * D[j + p * n] * G[1][i + p * n + k * nn] + D[k + p * n] * D[k + p * n] * G[2][i + j * n + p * nn];
                    const double di = D[i + i * n], dj = D[j + j * n], dk = D[k + k * n];
                    v += 2.0 * (di * dj * G[3][v0] + di * dk * G[4][v0] + dj * dk * G[5][v0]);
                    a[v0] = v;
                }
    }

    // Au = D^T G D u on one element, host (setup only: the hanging dofs of the exact diagonal)
    static void element_apply(double *Au, const double *u, const std::vector<DType> &D, const double *const G[NUM_GEOM_FACTS], int n, int dim)
    {
        const int nn = n * n, np = dim == 3 ? nn * n : nn;
        std::vector<double> g1(np), g2(np), g3(np);
        const int nk = dim == 3 ? n : 1;
        for (int k = 0; k < nk; k++)
            for (int j = 0; j < n; j++)
                for (int i = 0; i < n; i++)
                {
                    const int v = i + j * n + k * nn;
                    double d1 = 0.0, d2 = 0.0, d3 = 0.0;
                    for (int p = 0; p < n; p++)
                    {
                        d1 += D[p + i * n] * u[p + j * n + k * nn];
                        d2 += D[p + j * n] * u[i + p * n + k * nn];
                        if (dim == 3) d3 += D[p + k * n] * u[i + j * n + p * nn];
                    }
                    if (dim == 3)
                    {
                        g1[v] = G[0][v] * d1 + G[3][v] * d2 + G[4][v] * d3;
                        g2[v] = G[3][v] * d1 + G[1][v] * d2 + G[5][v] * d3;
                        g3[v] = G[4][v] * d1 + G[5][v] * d2 + G[2][v] * d3;
                    }
                    else
                    {
                        g1[v] = G[0][v] * d1 + G[2][v] * d2;
                        g2[v] = G[2][v] * d1 + G[1][v] * d2;
                    }
                }
        for (int k = 0; k < nk; k++)
            for (int j = 0; j < n; j++)
                for (int i = 0; i < n; i++)
                {
                    double a1 = 0.0, a2 = 0.0, a3 = 0.0;
                    for (int p = 0; p < n; p++)
                    {
                        a1 += D[i + p * n] * g1[p + j * n + k * nn];
                        a2 += D[j + p * n] * g2[i + p * n + k * nn];
                        if (dim == 3) a3 += D[k + p * n] * g3[i + j * n + p * nn];
                    }
                    Au[i + j * n + k * nn] = a1 + a2 + a3;
                }
    }

    void ensure_jacobi()
    {
        if (jacobi_dinv.ptr()) return;
        CSR_Matrix<DType> &Q = subdomain_operator.Q;
        const bool had_host = not Q.ptr_hst.empty();
        if (not had_host) Q.download_host();
        const int nse = subdomain_operator.num_extended_dofs, ns = subdomain_operator.num_dofs, nI = num_interface_dofs;
        std::vector<double> diag_ext(std::max(nse, 1), 0.0);
        std::vector<double> a, w, Aw, Gh[NUM_GEOM_FACTS];
        struct Entry
        {
            int dof, point;
            double weight;
        };
        std::vector<Entry> ent;
        for (auto &ll : subdomain_operator.level_lists)
        {
            const int n = ll.poly_degree + 1, np = (int)std::lround(std::pow(n, dim));
            const size_t total = (size_t)ll.num_elements * np;
            for (int g = 0; g < NUM_GEOM_FACTS; g++)
            {
                Gh[g].resize(total);
                if (total) FDD_CALL(fdd_memcpy_d2h(Gh[g].data(), ll.G[g], total * sizeof(double), fdd::dev().stream));
            }
            const std::vector<DType> &D = D_hat[ll.level].first;
            a.resize(np);
            w.resize(np);
            Aw.resize(np);
            for (int e = 0; e < ll.num_elements; e++)
            {
                const double *Ge[NUM_GEOM_FACTS];
                for (int g = 0; g < NUM_GEOM_FACTS; g++) Ge[g] = Gh[g].data() + (size_t)e * np;
                element_diagonal(a.data(), D, Ge, n, dim);
                const int base = ll.first_offset + e * np;
                bool plain = true; // every point of the element has at most one entry, of weight one: distinct dofs, no interpolation
                for (int p = 0; p < np and plain; p++)
                {
                    const int t0 = Q.ptr_hst[base + p], t1 = Q.ptr_hst[base + p + 1];
                    plain = t1 - t0 == 0 or (t1 - t0 == 1 and Q.val_hst[t0] == (DType)1.0);
                }
                if (plain)
                {
                    for (int p = 0; p < np; p++)
                        for (int t = Q.ptr_hst[base + p]; t < Q.ptr_hst[base + p + 1]; t++) diag_ext[Q.col_hst[t]] += Q.val_hst[t] * Q.val_hst[t] * a[p];
                    continue;
                }
                ent.clear();
                for (int p = 0; p < np; p++)
                    for (int t = Q.ptr_hst[base + p]; t < Q.ptr_hst[base + p + 1]; t++) ent.push_back(Entry{Q.col_hst[t], p, (double)Q.val_hst[t]});
                std::sort(ent.begin(), ent.end(), [](const Entry &x, const Entry &y) { return x.dof != y.dof ? x.dof < y.dof : x.point < y.point; });
                for (size_t b = 0; b < ent.size();)
                {
                    size_t e2 = b + 1;
                    while (e2 < ent.size() and ent[e2].dof == ent[b].dof) e2++;
                    if (e2 == b + 1)
                        diag_ext[ent[b].dof] += ent[b].weight * ent[b].weight * a[ent[b].point];
                    else
                    {
                        std::fill(w.begin(), w.end(), 0.0);
                        for (size_t t = b; t < e2; t++) w[ent[t].point] += ent[t].weight;
                        element_apply(Aw.data(), w.data(), D, Ge, n, dim);
                        double v = 0.0;
                        for (size_t t = b; t < e2; t++) v += ent[t].weight * Aw[ent[t].point];
                        diag_ext[ent[b].dof] += v;
                    }
                    b = e2;
                }
            }
        }
        if (not had_host) Q.release_host();
        // the unique dofs: [subdomain regular | interface] take the element sums; the superdomain's regular dofs (the
        // subdomain's extended dofs among them) take their rows of A (operator_dofs / subdomain.tpp:3951)
        jacobi_diag_hst.assign(std::max(num_dofs, 1), 1.0);
        for (int d = 0; d < std::min(ns, num_dofs); d++) jacobi_diag_hst[d] = diag_ext[d];
        for (size_t d = 0; d < std::min(shift_dofs_hst.size(), jacobi_diag_hst.size()); d++) jacobi_diag_hst[d] += shift_dofs_hst[d]; // the Helmholtz term is diagonal
        if (superdomain_operator.num_extended_dofs > 0)
        {
            const CSR_Matrix<DType> &A = superdomain_operator.A;
            for (int d = ns; d < num_dofs; d++)
            {
                const int row = nI + (d - ns);
                double v = 0.0;
                for (int t = A.ptr_hst[row]; t < A.ptr_hst[row + 1]; t++)
                    if (A.col_hst[t] == row) v = A.val_hst[t];
                jacobi_diag_hst[d] = v;
            }
        }
        std::vector<double> inv(jacobi_diag_hst.size());
        for (size_t d = 0; d < inv.size(); d++)
        {
            if (not(jacobi_diag_hst[d] > 0.0))
            {
                fprintf(stderr, "ERROR: Subdomain point-Jacobi: dof %zu has diagonal %g\n", d, jacobi_diag_hst[d]);
                exit(EXIT_FAILURE);
            }
            inv[d] = 1.0 / jacobi_diag_hst[d];
        }
        jacobi_dinv = fdd::dev().malloc<DType>(inv.size());
        jacobi_dinv.copyFrom(inv.data(), inv.size() * sizeof(DType));
        jacobi_dinv_f32 = fdd::to_float(inv);
    }

    // the preconditioner slot of the reference-shaped loops with point-Jacobi in it: low_order_preconditioner
    // (subdomain.tpp:3987-4159) with the V-cycle replaced by a division by the diagonal
    void jacobi_preconditioner(fdd::memory &z, fdd::memory &r)
    {
        ensure_jacobi();
        fdd::memory r_sub_l = r.slice(0, subdomain_operator.num_points);
        fdd::memory z_sub_l = z.slice(0, subdomain_operator.num_points);
        subdomain_operator.Qt.multiply(work_dev[0], r_sub_l);
        copy_tail(work_dev[0], r);
        fdd::memory *t = &work_dev[0];
        if (not Qt_int.is_identity)
        {
            Qt_int.multiply(work_dev[1], work_dev[0]);
            t = &work_dev[1];
        }
        FDD_CALL(fdd_vector_diagonal_scaling_dev(work_dev[2].as<double>(), jacobi_dinv.as<double>(), nullptr, t->template as<double>(), num_dofs, fdd::dev().stream));
        if (Q_int.is_identity)
            subdomain_operator.Q.multiply(z_sub_l, work_dev[2]);
        else
        {
            Q_int.multiply(work_dev[0], work_dev[2]);
            subdomain_operator.Q.multiply(z_sub_l, work_dev[0]);
            copy_tail_back(z, work_dev[0]);
        }
    }

    // ------------------------------------------------------------------
    // The composite in DOF SPACE: what gmres_dofs works on when the region is a composite.
    //
    // The reference's inner Krylov vectors are [region points | superdomain dofs] and every step goes through
    // Qt, QQt_int / Q_int / Qt_int and Q (subdomain.tpp:3969-4004, 4277-4307).  All of that only ever looks at the
    // UNIQUE dofs (norm_weight is their indicator, QQt_int copies from them), so the iteration is carried on
    //     U = [ subdomain dofs: regular | interface ][ superdomain regular dofs ]          (num_dofs values)
    // and the numbering of composite.hpp makes the copies fall into place without index maps:
    //   - the subdomain's extended dofs are the superdomain's first regular dofs, in the same order:
    //     U[0 : sub_ext_dofs) IS the vector Q acts on;
    //   - the superdomain's interface dofs are the subdomain's last dofs: U[sub_dofs - interface : num_dofs) is
    //     [interface | regular] of the vector A acts on; its extended dofs (copies of subdomain dofs) are gathered
    //     right behind it: W = [ U | superdomain-extended copies | hanging-point values ].
    // Non-conforming rows of Q: a hanging point's value is S * U (S = its J_cf row), computed into the tail of W
    // before the element kernels run, which then read every point through ONE index array (gather-on-load, the
    // same fused kernel as the conforming path); on the way back the element results are gathered by a boolean
    // matrix (dofs, then hanging points) and the hanging values are folded in with S^T.
    // Operator application: indexed copy (small) + S (small) + stiffness per level list + boolean gather + S^T
    // (small) + the superdomain rows of A (small).  Inner products are plain dots over num_dofs.
    // ------------------------------------------------------------------
    void setup_composite_dofs()
    {
        const fdd::composite::Composite &c = comp;
        const int NP = c.num_sub_ext_points, nse = c.sub_num_ext_dofs, ns = c.sub_num_dofs, nI = c.num_interface_dofs, nu = c.sup_num_dofs, nue = c.sup_num_ext_dofs;
        comp_dofs_ready = false;
        if (dim != 3) return;
        for (auto &ll : subdomain_operator.level_lists)
            if (ll.poly_degree > 15) return;
        // the layout above needs the subdomain's extended dofs to be the superdomain's leading regular dofs
        for (int d = ns; d < nse; d++)
            if (c.Q_int_col[d] != d) return;
        n_sup_copies = nue - nu;
        const CSR_Matrix<DType> &Q = subdomain_operator.Q;
        std::vector<int> index(NP, -1), slave_point;
        for (int p = 0; p < NP; p++)
        {
            if (c.point_dof[p] >= 0)
                index[p] = c.point_dof[p];
            else if (Q.ptr_hst[p + 1] > Q.ptr_hst[p])
                slave_point.push_back(p);
        }
        n_slaves = (int)slave_point.size();
        slave_base = num_dofs + n_sup_copies;
        W_len = slave_base + n_slaves;
        {
            std::vector<int> sp(n_slaves + 1, 0), sc;
            std::vector<DType> sv;
            for (int h = 0; h < n_slaves; h++)
            {
                const int p = slave_point[h];
                index[p] = slave_base + h;
                for (int k = Q.ptr_hst[p]; k < Q.ptr_hst[p + 1]; k++)
                {
                    sc.push_back(Q.col_hst[k]);
                    sv.push_back(Q.val_hst[k]);
                }
                sp[h + 1] = (int)sc.size();
            }
            if (n_slaves > 0)
            {
                S_slave.assemble_from_csr(n_slaves, nse, sp.data(), sc.data(), sv.data());
                // S^T by rows, entries in hanging-point order, empty rows left out
                std::vector<int> count(nse, 0);
                for (int c2 : sc) count[c2]++;
                std::vector<int> rows_of, slot(nse, -1);
                for (int d = 0; d < nse; d++)
                    if (count[d] > 0)
                    {
                        slot[d] = (int)rows_of.size();
                        rows_of.push_back(d);
                    }
                const int m = (int)rows_of.size();
                std::vector<int> tp(m + 1, 0);
                for (int r = 0; r < m; r++) tp[r + 1] = tp[r] + count[rows_of[r]];
                std::vector<int> tc(sc.size()), fill(tp.begin(), tp.end() - 1);
                std::vector<DType> tv(sc.size());
                for (int h = 0; h < n_slaves; h++)
                    for (int k = sp[h]; k < sp[h + 1]; k++)
                    {
                        const int at = fill[slot[sc[k]]]++;
                        tc[at] = h;
                        tv[at] = sv[k];
                    }
                St_slave.assemble_from_csr(m, n_slaves, tp.data(), tc.data(), tv.data());
                st_rows = fdd::dev().malloc<int>(std::max(m, 1));
                st_rows.copyFrom(rows_of.data(), (size_t)m * sizeof(int));
                st_tmp = fdd::dev().malloc<DType>(std::max(m, 1));
            }
            slave_vals = fdd::dev().malloc<DType>(std::max(n_slaves, 1));
        }
        // every region point through one index array into W
        point_dof_dev = fdd::dev().malloc<int>(std::max(NP, 1));
        point_dof_dev.copyFrom(index.data(), (size_t)NP * sizeof(int));
        // boolean gather: row d < nse collects the points of dof d, row nse + h is hanging point h
        {
            const int rows = nse + n_slaves;
            std::vector<int> gp(rows + 1, 0);
            for (int p = 0; p < NP; p++)
                if (index[p] >= 0) gp[(index[p] < nse ? index[p] : nse + (index[p] - slave_base)) + 1]++;
            for (int r = 0; r < rows; r++) gp[r + 1] += gp[r];
            std::vector<int> gc(gp[rows]), fill(gp.begin(), gp.end() - 1);
            for (int p = 0; p < NP; p++)
                if (index[p] >= 0) gc[fill[index[p] < nse ? index[p] : nse + (index[p] - slave_base)]++] = p;
            std::vector<DType> gv(gc.size(), 1.0);
            G_unit.assemble_from_csr(rows, NP, gp.data(), gc.data(), gv.data());
            G_unit.release_host();
            // the rows of the rank's own dofs restricted to ring points, empty rows left out: with the own part of a
            // right-hand side taken from the outer solve's assembled residual only these few sums are left to form
            const int n_own = c.num_own_dofs;
            std::vector<int> rows_of, rp2(1, 0), rc2;
            for (int d = 0; d < n_own; d++)
            {
                const size_t before = rc2.size();
                for (int k = gp[d]; k < gp[d + 1]; k++)
                    if (gc[k] >= own_points) rc2.push_back(gc[k]);
                if (rc2.size() > before)
                {
                    rows_of.push_back(d);
                    rp2.push_back((int)rc2.size());
                }
            }
            if (not rows_of.empty())
            {
                std::vector<DType> rv2(rc2.size(), 1.0);
                G_ring.assemble_from_csr((int)rows_of.size(), NP, rp2.data(), rc2.data(), rv2.data());
                ring_rows = fdd::dev().malloc<int>(rows_of.size());
                ring_rows.copyFrom(rows_of.data(), rows_of.size() * sizeof(int));
                ring_tmp = fdd::dev().malloc<DType>(rows_of.size());
            }
        }
        {
            std::vector<int> src(std::max(n_sup_copies, 1), 0);
            for (int k = 0; k < n_sup_copies; k++) src[k] = c.Q_int_col[(size_t)nse + nu + k];
            copy_src = fdd::dev().malloc<int>(std::max(n_sup_copies, 1));
            copy_src.copyFrom(src.data(), src.size() * sizeof(int));
        }
        if (nu - nI > 0)
        {
            const fdd::low_order::HostCSR &A = c.A_sup;
            std::vector<int> ap(nu - nI + 1, 0);
            for (int i = nI; i < nu; i++) ap[i - nI + 1] = ap[i - nI] + (A.ptr[i + 1] - A.ptr[i]);
            A_sup_reg.assemble_from_csr(nu - nI, nue, ap.data(), A.col.data() + A.ptr[nI], A.val.data() + A.ptr[nI]);
        }
        comp_dofs_ready = true;
    }

    int dof_space_size() const { return is_composite ? num_dofs : subdomain_operator.num_extended_dofs; }
    int dof_alloc_size() const { return is_composite ? W_len : subdomain_operator.num_extended_dofs; }

    // the right-hand side of the composite in dof space from the tree-exchanged composite vector T r (subdomain.tpp:4566-4646)
    // own_assembled: the sums over the rank's OWN points of every own dof, already formed by the caller (the outer
    // solve's node residual, which it keeps assembled): then only the ring points are gathered here
    void composite_rhs_dofs(fdd::memory &fa_out, fdd::memory &Tr, const double *own_assembled = nullptr)
    {
        const int nse = subdomain_operator.num_extended_dofs, ns = subdomain_operator.num_dofs, nI = num_interface_dofs, n_reg = superdomain_operator.num_dofs - nI;
        if (own_assembled)
        {
            const int n_own = comp.num_own_dofs;
            FDD_CALL(fdd_memcpy_d2d(fa_out.ptr(), own_assembled, (size_t)n_own * sizeof(DType), fdd::dev().stream));
            G_unit.gather_scatter(nullptr, fa_out.as<double>(), Tr.as<double>(), nullptr, nullptr, n_own, nse, 1);
            if (G_ring.num_rows > 0)
            {
                G_ring.multiply(ring_tmp, Tr);
                FDD_CALL(fdd_scatter_add_indexed(fa_out.as<double>(), ring_rows.template as<int>(), ring_tmp.as<double>(), G_ring.num_rows, fdd::dev().stream));
            }
        }
        else
            G_unit.gather_scatter(nullptr, fa_out.as<double>(), Tr.as<double>(), nullptr, nullptr, 0, nse, 1);
        if (n_slaves > 0)
        {
            G_unit.gather_scatter(nullptr, slave_vals.as<double>() - nse, Tr.as<double>(), nullptr, nullptr, nse, nse + n_slaves, 1);
            St_slave.multiply(st_tmp, slave_vals);
            FDD_CALL(fdd_scatter_add_indexed(fa_out.as<double>(), st_rows.template as<int>(), st_tmp.as<double>(), St_slave.num_rows, fdd::dev().stream));
        }
        if (n_reg > 0)
        {
            fdd::memory dst = fa_out.slice(ns, n_reg);
            dst.copyFrom(Tr.slice(subdomain_operator.num_points + nI, n_reg), (size_t)n_reg * sizeof(DType));
        }
    }

    // u on the rank's own points from the dof-space solution (Q u~ restricted to level 0)
    void composite_solution_points(fdd::memory &u_l, fdd::memory &ua_in)
    {
        if (n_slaves > 0)
        {
            fdd::memory slaves = ua_in.slice(slave_base, n_slaves);
            S_slave.multiply(slaves, ua_in);
        }
        FDD_CALL(fdd_gather_indexed(u_l.as<double>(), ua_in.as<double>(), point_dof_dev.template as<int>(), nullptr, own_points, fdd::dev().stream));
    }


    // ------------------------------------------------------------------
    // Single-precision preconditioner: the reference instantiates Subdomain<PTYPE> with PTYPE = Float
    // (config.hpp:19-20, poisson.cpp:206; run.py:157 sweeps Float = float), i.e. the WHOLE inner solve -- element
    // stiffness, gather, Krylov vectors, V-cycle -- on float data, with the casts of subdomain.okl:268-282 at its two
    // ends.  Here the same switch is taken at run time (set_precision(32)): the dof-space inner GMRES below works on
    // float copies of the geometric factors, D_hat, the hanging-point rows and the superdomain operator, its vectors
    // are float, its V-cycle is the f32 cycle of amg.hpp entered and left in float.  Device-resident scalars
    // (Hessenberg column, Givens state, 1/norm scales) and the accumulators of the dots stay double.
    // ------------------------------------------------------------------
    struct SinglePrecision
    {
        bool ready = false;
        amg::Csr32 S, St, Asup;                                  // S_slave, St_slave, A_sup_reg
        fdd::memory q_pts, slaves, st_tmp;
    } sp;

    void prepare_single_precision()
    {
        if (sp.ready) return;
        void *stream = fdd::dev().stream;
        for (auto &ll : subdomain_operator.level_lists)
        {
            const size_t np = ll.num_points();
            for (int g = 0; g < NUM_GEOM_FACTS; g++)
            {
                ll.G32[g] = fdd::dev().malloc<float>(std::max<size_t>(np, 1));
                FDD_CALL(fdd_sub_copy_f32_f64(ll.G32[g].template as<float>(), ll.G[g], (int)np, stream));
            }
        }
        for (auto &ll : subdomain_operator.level_lists)
        {
            ll.D_hat32 = fdd::to_float(D_hat[ll.level].first);
            fdd::check_lean_table32(ll, D_hat[ll.level].first);
        }
        auto plan32 = [](amg::Csr32 &M32, CSR_Matrix<DType> &M) {
            if (M.num_rows == 0 or M.num_nnz == 0) return;
            M32.val = fdd::to_float(M.val_hst);
            M32.plan = fdd::make_csr_plan(M.ptr_hst.data(), M.num_rows, M.num_cols, M.num_nnz, true);
        };
        if (is_composite)
        {
            plan32(sp.S, S_slave);
            plan32(sp.St, St_slave);
            plan32(sp.Asup, A_sup_reg);
        }
        sp.q_pts = fdd::dev().malloc<float>(std::max(subdomain_operator.num_points, 1));
        sp.slaves = fdd::dev().malloc<float>(std::max(n_slaves, 1));
        sp.st_tmp = fdd::dev().malloc<float>(std::max(St_slave.num_rows, 1));
        sp.ready = true;
    }

    // y = M x with one of the composite's small matrices; a matrix without entries leaves the float y alone
    static void multiply(CSR_Matrix<DType> &M, amg::Csr32 &, double *y, const double *x) { M.multiply(y, x); }
    static void multiply(CSR_Matrix<DType> &M, amg::Csr32 &M32, float *y, const float *x)
    {
        if (M32.plan) FDD_CALL(fdd_csr_plan_matvec_to_f32(M32.plan.get(), y, nullptr, M.ptr.template as<int>(), M.col.template as<int>(), M32.val.template as<float>(), x, 1.0f, 0.0f, fdd::dev().stream));
    }

    // q (points) = A_local (Q (s z~)), s = *scale_dev when given (a basis vector kept unnormalised): one launch per level
    // list, in double or on the float data of prepare_single_precision
    template <typename Real>
    void stiffness_from_dofs(Real *q, const Real *za, const double *scale_dev = nullptr)
    {
        for (auto &ll : subdomain_operator.level_lists) fdd::apply_gather(ll, q, za, point_dof_dev.template as<int>(), scale_dev, subdomain_operator.num_extended_dofs, stiffness);
    }

  public:
    // ---- rows of Qt completed by the stiffness kernel (flag "assemble_in_stiffness", assembly_classes.hpp) ----
    // The classes of Qt's rows, from Qt's own arrays: made when first asked for and again after every set-up (both forms of
    // set-up clear them where they rebuild the lists and Qt)
    fdd::AssemblyClasses assembly;
    void assembly_build()
    {
        CSR_Matrix<DType> &Qt = subdomain_operator.Qt;
        std::vector<int> ptr((size_t)Qt.num_rows + 1, 0), col((size_t)Qt.num_nnz);
        if (Qt.num_nnz > 0) // the host mirrors are dropped after set-up: the device arrays are the matrix
        {
            Qt.ptr.copyTo(ptr.data(), ptr.size() * sizeof(int));
            Qt.col.copyTo(col.data(), col.size() * sizeof(int));
        }
        assembly.build(ptr.data(), col.data(), Qt.num_rows, subdomain_operator.num_points, point_dof, subdomain_operator.level_lists);
    }
    // Why operator_dofs keeps the point buffer and the whole gather in double (nullptr: it does not).  A handful of
    // comparisons per call once the classes are on the device
    const char *assembly_obstacle()
    {
        if (not stiffness.assemble_in_stiffness) return "the flag is off";
        if (precision != 64) return "the inner solve runs in float";
        if (is_composite) return "a composite region";
        if (not norm_weight_is_one) return "the gather is weighted";
        if (subdomain_operator.level_lists.empty() or subdomain_operator.Qt.num_nnz == 0 or subdomain_operator.Qt.num_rows != subdomain_operator.num_extended_dofs or not subdomain_operator.Qt.unit_values) return "no boolean gather over every dof";
        for (auto &ll : subdomain_operator.level_lists)
            if (not fdd::direct_lines_apply(ll, stiffness)) return "a list does not run the degree-7 line form";
        if (not assembly.built) assembly_build();
        if (not assembly.ensure_device()) return assembly.unusable.c_str();
        return nullptr;
    }

  private:
    // y (dofs) = [Qt A_L Q | A_sup] (s x~): the operator of the inner iteration on a dof vector.  x~ is one of the
    // Krylov vectors; in a composite its allocation carries the copies and hanging values behind the dofs (W), which
    // are written here.  With a Helmholtz shift set (set_shift; conforming regions only) the zeroth-order term follows:
    // y += c .* (s x~), one more pass over the dofs.
    template <typename Real>
    void operator_dofs(Real *y, Real *x, const double *scale_dev = nullptr)
    {
        stiffness_operator_dofs(y, x, scale_dev);
        if (shift_indexed())
            fdd::ops::shift_add_indexed(y, (std::is_same<Real, float>::value ? shift_support.values_f32 : shift_support.values).template as<Real>(), shift_support.index.template as<int>(), shift_support.count, scale_dev, x, dof_space_size(), fdd::dev().stream);
        else if (shift_active())
            fdd::ops::shift_add(y, (std::is_same<Real, float>::value ? shift_dofs_f32 : shift_dofs).template as<Real>(), scale_dev, x, dof_space_size(), fdd::dev().stream);
    }

    template <typename Real>
    void stiffness_operator_dofs(Real *y, Real *x, const double *scale_dev)
    {
        constexpr bool f32 = std::is_same<Real, float>::value;
        void *stream = fdd::dev().stream;
        Real *q = (f32 ? sp.q_pts : q_k).template as<Real>();
        const int nse = subdomain_operator.num_extended_dofs;
        if (not is_composite)
        {
            if constexpr (not f32)
                if (y != x and assembly_obstacle() == nullptr)
                {
                    // the line kernel completes the single and pair rows of y itself; the general rows' points go through q
                    for (auto &ll : subdomain_operator.level_lists) fdd::apply_gather_direct(ll, q, y, x, assembly.point_class_dof_dev.template as<int>(), scale_dev, nse, stiffness);
                    assembly.gather_general(y, q);
                    return;
                }
            stiffness_from_dofs(q, x, scale_dev);
            if constexpr (f32)
                subdomain_operator.Qt.gather(y, q, 0, nse); // the float gather takes no norm weight
            else
                subdomain_operator.Qt.gather(y, q, 0, nse, norm_weight_is_one ? nullptr : norm_weight.as<double>());
            return;
        }
        const int ns = subdomain_operator.num_dofs, nI = num_interface_dofs, n_reg = superdomain_operator.num_dofs - nI;
        if (n_sup_copies > 0) fdd::ops::gather_indexed(x + num_dofs, x, copy_src.template as<int>(), n_sup_copies, stream);
        if (n_slaves > 0) multiply(S_slave, sp.S, x + slave_base, x);
        stiffness_from_dofs(q, x, scale_dev);
        G_unit.gather(y, q, 0, nse);
        if (n_slaves > 0)
        {
            Real *sl = (f32 ? sp.slaves : slave_vals).template as<Real>(), *st = (f32 ? sp.st_tmp : st_tmp).template as<Real>();
            G_unit.gather(sl - nse, q, nse, nse + n_slaves);
            multiply(St_slave, sp.St, st, sl);
            fdd::ops::scatter_add_indexed(y, st_rows.template as<int>(), st, St_slave.num_rows, stream);
        }
        if (n_reg > 0)
        {
            multiply(A_sup_reg, sp.Asup, y + ns, x + (ns - nI));
            if (scale_dev) fdd::ops::scaling_dev(y + ns, scale_dev, y + ns, n_reg, stream);
        }
    }

  public:
    int precision = 64; // the reference's PTYPE / Float: 64 = double, 32 = float (set_precision)

    // 32: the dof-space inner solve and its V-cycle run in float; 64: double (the V-cycle's own precision can still be
    // lowered alone through amg_hierarchy.set_precision, AMG/config.hpp:4)
    bool set_precision(int bits)
    {
        if (bits != 64 and bits != 32) return false;
        if (bits == 32 and not(dim == 3 and device_bookkeeping and ((assembled_inner and can_assemble()) or composite_dof_space()))) return false;
        precision = bits;
        if (amg_hierarchy.ready())
        {
            amg_hierarchy.set_f32_io(false);
            if (not amg_hierarchy.set_precision(bits)) return false;
        }
        return true;
    }

  private:
    // a new inner solve starts
    void begin_inner_solve()
    {
        residual_history.clear();
        history_pending = false; // a lazy solve before this one (pcg_steps) may have left its history on the device: it is not this solve's
    }

  public:
    bool composite_dof_space() const { return is_composite and comp_dofs_ready and assembled_inner and device_bookkeeping and num_vectors <= FDD_MULTI_MAX; }
    int own_dofs() const { return is_composite ? comp.num_own_dofs : subdomain_operator.num_extended_dofs; }

    // z~ = M^-1 r for the node-space outer solve: r is the outer residual on the rank's own points (the degree tree
    // and the ring / superdomain exchange start from it), the result the dof-space correction (its leading own_dofs()
    // entries follow the Domain's node order)
    void gmres_composite_dofs(fdd::memory &ua_out, fdd::memory &r_pts, bool print_history = true, bool use_relative = false, const double *own_assembled = nullptr, const fdd::InnerSolveHints &hints = {})
    {
        fdd::memory &fa = krylov64.fa;
        if (not fa.ptr()) fa = fdd::dev().malloc<DType>(std::max(dof_alloc_size(), 1));
        tree_operator(f, r_pts);
        composite_rhs_dofs(fa, f, own_assembled);
        gmres_dofs_device(ua_out, fa, print_history, use_relative, hints);
    }
    fdd::memory new_dof_vector() { return fdd::dev().malloc<DType>(std::max(dof_alloc_size(), 1)); }
    // the two exchanges of tree_operator alone, on their buffers' current contents (bench.py's communication timings)
    void comm_probe_coarse()
    {
        if (not is_composite or (fdd::comm().size == 1 and superdomain_operator.num_extended_dofs == 0)) return; // rank-uniform, like tree_exchange
        fdd::memory coarse = work_dev[0].slice(levels[num_levels - 1].offset, coarse_pad);
        fdd::comm().allgather(coarse.ptr(), coarse_all.ptr(), (size_t)coarse_pad * sizeof(DType));
    }
    void comm_probe_ring()
    {
        if (not is_composite) return;
        fdd::comm().exchange(exchange_ops.data(), (int)exchange_ops.size());
    }
    // ring pull and coarse blocks in one group, as tree_exchange issues them by default
    void comm_probe_ring_and_coarse()
    {
        if (not is_composite) return;
        fdd::comm().exchange(exchange_ops_folded.data(), (int)exchange_ops_folded.size());
    }
    double comm_ring_and_coarse_bytes() const
    {
        double b = 0.0;
        for (const fdd::ExchangeOp &op : exchange_ops_folded) b += (double)op.send_bytes;
        return b;
    }
    double comm_coarse_bytes() const { return is_composite ? (double)coarse_pad * sizeof(DType) * fdd::comm().size : 0.0; }
    double comm_ring_bytes() const
    {
        double b = 0.0;
        for (const fdd::ExchangeOp &op : exchange_ops) b += (double)op.send_bytes;
        return b;
    }
    // where the outer solve keeps its point-space residual: the own-points head of the tree vector, so that
    // tree_operator finds level 0 in place
    fdd::memory tree_points() { return f.slice(0, own_points); }

  private:
    // A hierarchy that amg_build made is built again after a change that reaches the low-order matrix (operator_changed,
    // amg_rebuild); one that was handed in is the caller's and stays.  A sweep's reader sees what the change costs
    void rebuild_own_hierarchy(const char *change)
    {
        if (not(amg_hierarchy.ready() and amg_built_here)) return;
        const int nl = amg_build(amg_build_options);
        rstdout("Low-order preconditioner assembled again (%s): %d levels, %.3f s\n", change, nl, amg_setup_seconds);
    }

  public:
    const char *data_type = "double";

    // Solver (subdomain.hpp:228-238)
    int num_iterations = 0;
    int num_vectors = 4;
    int max_iterations = 4;
    bool use_preconditioner = true; // subdomain.hpp:231; the hierarchy is handed in (amg_add_level) or built on first use (amg_build)
    bool use_jacobi = false;        // with use_preconditioner == false: point-Jacobi in the preconditioner slot instead of the identity (labelled option of this build)
    const std::vector<double> &jacobi_diagonal()
    {
        ensure_jacobi();
        return jacobi_diag_hst;
    }

    // The operator under the diagonal has changed: the diagonal, its inverses and the eigenvalue bound of the Chebyshev inner
    // solve are made again at their next use, and the first step's scaling with them (operator_generation).  Which change
    // brings which arguments is said once, in fdd_host_capi.cpp (operator_changed there, the only caller).  D != nullptr: the
    // table of the level of that degree, whose host copy this class keeps (the device table is the Domain's own).
    // low_order_term != nullptr: the change reaches the low-order matrix, and a hierarchy that amg_build made is built again
    // now; the text names the change in the printed line.
    void operator_changed(int degree = -1, const double *D = nullptr, int n = 0, const char *low_order_term = nullptr)
    {
        for (int l = 0; D != nullptr and l < num_levels; l++)
            if (poly_degree[l] == degree) D_hat[l].first.assign(D, D + (size_t)n * n);
        for (auto &ll : subdomain_operator.level_lists)
            if (D != nullptr and poly_degree[ll.level] == degree)
            {
                fdd::check_lean_table(ll, D_hat[ll.level].first); // the Domain has uploaded this table
                if (not ll.D_hat32.ptr()) continue;
                ll.D_hat32 = fdd::to_float(D_hat[ll.level].first); // the float solve was prepared under the table as it was: its copy and its verdict follow
                fdd::check_lean_table32(ll, D_hat[ll.level].first);
            }
        jacobi_dinv = jacobi_dinv_f32 = fdd::memory();
        jacobi_diag_hst.clear();
        cheby.lambda = 0.0;
        operator_generation++;
        if (low_order_term != nullptr) rebuild_own_hierarchy(low_order_term);
    }

    // ---- Helmholtz shift: the inner operator is Qt A_L Q + diag(c), c >= 0 over the dofs -- a LABELLED OPTION of this build ----
    // c is the Domain's node vector (Domain::set_shift) in this class's dof numbering, kept in both precisions and on the
    // host (the exact diagonal and the low-order matrix take it from there).  An empty c: off.  The caller follows with
    // operator_changed.
    std::vector<double> shift_dofs_hst;
    fdd::memory shift_dofs, shift_dofs_f32;
    fdd::boundary::ShiftSupport shift_support; // the entries of c that are not zero (boundary.hpp); flag "indexed_shift"
    bool indexed_shift = fdd::missing_indexed_shift_entry() == nullptr;
    bool shift_active() const { return not shift_dofs_hst.empty(); }
    bool shift_indexed() const { return shift_active() and shift_support.applies(indexed_shift, dof_space_size()); }
    void set_shift(const std::vector<double> &c)
    {
        shift_dofs = shift_dofs_f32 = fdd::memory();
        shift_support.release();
        shift_dofs_hst = c;
        if (c.empty()) return;
        shift_support.build(c);
        shift_dofs = fdd::dev().malloc<DType>(c.size());
        shift_dofs.copyFrom(c.data(), c.size() * sizeof(DType));
        shift_dofs_f32 = fdd::to_float(c);
    }

    // ---- a diffusivity per point (diffusivity.hpp): the inner operator is Qt D^T [kappa G] D Q -- a LABELLED OPTION of this build ----
    // On one rank without a composite the inner operator is the fine level's own list on the Domain's own arrays, which
    // Domain::set_diffusivity has just rewritten: what this class derived from them is derived again (the list's verdicts and
    // float copies), the list takes the Domain's members of the coefficient instance as views, and the values are kept for
    // the low-order matrix; the caller follows with operator_changed.  The classes of the rows of
    // Qt (assembly) do not depend on the factors or on the kernel's instance and stay.  A Helmholtz shift is independent of
    // all this and keeps the unscaled mass.  kappa == nullptr: cleared.
    std::vector<double> diffusivity_hst;
    bool diffusivity_active() const { return not diffusivity_hst.empty(); }
    void set_diffusivity(const double *kappa, size_t n, const fdd::LevelList &domain_list)
    {
        diffusivity_hst.assign(kappa, kappa + (kappa != nullptr ? n : 0));
        for (auto &ll : subdomain_operator.level_lists)
        {
            fdd::diffusivity::refresh_list(ll);
            fdd::diffusivity::share_coef(ll, domain_list);
        }
    }

    // why a solve of this problem would not carry the shift (it enters through operator_dofs alone), or nullptr
    const char *helmholtz_refusal() const
    {
        if (is_composite) return "a Helmholtz shift needs a conforming region: this Subdomain is a composite";
        if (not dof_space_available()) return "a Helmholtz shift needs the dof-space inner solve: a 3-D region with assembled_inner_solve = 1";
        if (not norm_weight_is_one) return "a Helmholtz shift needs an unweighted gather in the inner operator";
        if (not chebyshev() and not(device_bookkeeping and num_vectors <= FDD_MULTI_MAX)) return "a Helmholtz shift needs the inner GMRES with its bookkeeping on the device: the host-bookkeeping loop does not go through operator_dofs";
        return nullptr;
    }

    // ---- Chebyshev-Jacobi inner solve (chebyshev_dofs below): a LABELLED OPTION of this build, off by default ----
    int inner_solver = 0; // 0: the inner FCG / GMRES(m) as in the reference; 1: a fixed Chebyshev polynomial in D^-1 A
    bool chebyshev() const { return inner_solver == 1; }
    struct ChebyshevOptions
    {
        int order = 4;                   // m: m diagonal scalings, m - 1 operator applications
        double lower = 0.1, upper = 1.1; // the interval [lower, upper] * lambda
        int power_iterations = 25;
        bool use_kernels = true; // fdd_cheby_step where the library has it; false: composed from the entries that were there before
        bool fused = true;       // the step as the epilogue of the gather Qt where that applies (conforming region, unit norm weight)
        double lambda = 0.0;     // Rayleigh quotient of D^-1/2 A D^-1/2 after power_iterations steps; 0: not computed yet
    } cheby;
    template <typename Real>
    struct ChebyVectors
    {
        fdd::memory d, r, q, t, x, f; // direction, residual, A d, scratch of the composed step; x, f: the float solve's own
        fdd::memory w;                // 1 / (theta diag): the first step's scaling, rounded once more than fa / (theta diag) itself
        double w_theta = 0.0;
        int w_generation = -1, na = 0;
    };
    ChebyVectors<double> cheby64;
    ChebyVectors<float> cheby32;
    int operator_generation = 0; // counts operator_changed(): what was derived from the diagonal knows whether it still holds
    DType tolerance = 1.0e-12;
    DType epsilon = 1.0e-12;

    int num_vcycles = 1;
    int cheby_order = 2;
    int level_cutoff = 5; // kept for the interface; every level lives in HBM here (amg.hpp)
    amg::Hierarchy amg_hierarchy;

    // hand the hierarchy in, finest level first (stands in for subdomain.tpp:3474-3549)
    void amg_add_level(int n, const int *A_ptr, const int *A_col, const double *A_val, const double *D_val, const double *coefs, int n_coarse, const int *P_ptr, const int *P_col, const double *P_val)
    {
        amg_hierarchy.cheby_order = cheby_order;
        amg_hierarchy.num_vcycles = num_vcycles;
        amg_hierarchy.add_level(n, A_ptr, A_col, A_val, D_val, coefs, n_coarse, P_ptr, P_col, P_val);
    }
    void amg_finalize() { amg_hierarchy.finalize(); }

    // lambda_max(D A D) of a level matrix of the setup: low_order::max_eigenvalue_scaled's power iteration (same start
    // vector, same count) with the SpMV and the vector work on the device -- 25 passes over a level-0 matrix of a
    // gigabyte are 0.5 s on the host's memory bus and 10 ms here.  One scalar comes back at the end.
    double device_lambda_max(const fdd::low_order::HostCSR &M, const std::vector<double> &D, int iterations)
    {
        const int n = M.rows;
        const size_t nnz = (size_t)M.nnz();
        if (n == 0 or nnz == 0 or iterations <= 0) return 1.0;
        fdd::device_t &dv = fdd::dev();
        void *stream = dv.stream;
        static const bool timing = getenv("FDD_SETUP_TIMING") != nullptr;
        const auto clock = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        const double t0 = clock();
        fdd::memory ptr = dv.malloc<int>((size_t)n + 1), col = dv.malloc<int>(nnz), val = dv.malloc<double>(nnz), Dd = dv.malloc<double>(n);
        ptr.copyFrom(M.ptr.data(), ((size_t)n + 1) * sizeof(int));
        col.copyFrom(M.col.data(), nnz * sizeof(int));
        val.copyFrom(M.val.data(), nnz * sizeof(double));
        Dd.copyFrom(D.data(), (size_t)n * sizeof(double));
        if (timing and n > 100000) printf("low_order:   lambda_max on the device: matrix up %.3f s\n", clock() - t0);
        return device_lambda_max(n, M.ptr, ptr, col, val, Dd, iterations);
    }
    // the same on a matrix and a D that are in HBM already (ptr_hst: the host's copy of the row pointers)
    double device_lambda_max(int n, const std::vector<int> &ptr_hst, const fdd::memory &ptr, const fdd::memory &col, const fdd::memory &val, const fdd::memory &Dd, int iterations)
    {
        const size_t nnz = (size_t)ptr_hst[(size_t)n];
        if (n == 0 or nnz == 0 or iterations <= 0) return 1.0;
        fdd::device_t &dv = fdd::dev();
        void *stream = dv.stream;
        static const bool timing = getenv("FDD_SETUP_TIMING") != nullptr;
        const auto clock = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        const double t1 = clock();
        const fdd::csr_plan plan = fdd::make_csr_plan(ptr_hst.data(), n, n, (int)nnz);
        const double t2 = clock();
        const double lambda = device_power_iteration(n, 0, Dd, iterations, [&](fdd::memory &w, fdd::memory &t) {
            FDD_CALL(fdd_csr_plan_matvec(plan.get(), w.as<double>(), ptr.as<int>(), col.as<int>(), val.as<double>(), t.as<double>(), 1.0, 0.0, stream));
        });
        if (timing and n > 100000) printf("low_order:   lambda_max on the device: plan %.3f s, vectors and %d iterations %.3f s\n", t2 - t1, iterations, clock() - t2);
        return lambda;
    }
    // The Rayleigh quotient of S A S after `iterations` steps of low_order::max_eigenvalue_scaled's power iteration (same start
    // vector) on the device: six launches a step around apply(w, t), w = A t.  S: the diagonal scaling, n entries.  padded > 0:
    // t and w have that many entries (>= n) and t is cleared first, for an operator that reads behind the n.  One scalar
    // comes back at the end.
    template <typename Apply>
    static double device_power_iteration(int n, int padded, const fdd::memory &S, int iterations, Apply &&apply)
    {
        fdd::device_t &dv = fdd::dev();
        void *stream = dv.stream;
        const int nt = padded > 0 ? padded : n;
        fdd::memory v = dv.malloc<double>(n), vn = dv.malloc<double>(n), t = dv.malloc<double>(nt), w = dv.malloc<double>(nt);
        fdd::memory ws = dv.malloc<double>(fdd_reduce_workspace_doubles()), sc = dv.malloc<double>(2);
        {
            const std::vector<double> start = fdd::low_order::power_iteration_start(n);
            v.copyFrom(start.data(), (size_t)n * sizeof(double));
        }
        if (padded > 0) FDD_CALL(fdd_set_to_value(t.as<double>(), 0.0, nt, 0, stream));
        double *scp = sc.as<double>();
        for (int it = 0; it < iterations; it++)
        {
            FDD_CALL(fdd_sub_inner_product(scp, ws.as<double>(), v.as<double>(), v.as<double>(), n, stream));
            FDD_CALL(fdd_vector_scaling_rsqrt_dev(vn.as<double>(), scp, v.as<double>(), n, stream));                        // vn = v / |v|
            FDD_CALL(fdd_vector_diagonal_scaling_dev(t.as<double>(), S.as<double>(), nullptr, vn.as<double>(), n, stream)); // t = S vn
            apply(w, t);
            FDD_CALL(fdd_vector_diagonal_scaling_dev(v.as<double>(), S.as<double>(), nullptr, w.as<double>(), n, stream)); // v = S A S vn
            FDD_CALL(fdd_sub_inner_product(scp + 1, ws.as<double>(), v.as<double>(), vn.as<double>(), n, stream));
        }
        double lambda = 1.0;
        sc.slice(1, 1).copyTo(&lambda, sizeof(double));
        return lambda;
    }

    // Build the low-order FEM matrix of the region and an AMG hierarchy for it on the host and attach it
    // (stands in for subdomain.tpp:2749-3549, see low_order.hpp).  Returns the number of levels.
    // With amg_device_setup (conforming regions): the FEM matrix and every level coarsened on the lattice are built in
    // HBM (amg_device_setup.hpp) and stay there; the first level that is not is downloaded and the host loop
    // (low_order::build) continues from it, level index and lattice state kept.  Bit-identical either way.
    int amg_build(fdd::low_order::Options options, bool verbose = false)
    {
        if (dim != 3 or fine_mesh == nullptr or (poly_degree[0] < 2 and not is_composite))
        {
            fprintf(stderr, "ERROR: Subdomain::amg_build handles 3-D regions of degree >= 2\n");
            exit(EXIT_FAILURE);
        }
        amg_build_options = options; // kept: a later change of "amg_cheby_order" rebuilds with them (amg_rebuild)
        options.cheby_order = cheby_order;
        static const bool timing = getenv("FDD_SETUP_TIMING") != nullptr;
        const auto clock = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        const double t0 = clock();
        const bool on_device = amg_device_setup and not is_composite and not shift_active() and not diffusivity_active();
        if (amg_device_setup and shift_active()) rstdout("amg_device_setup: with a Helmholtz shift set the low-order hierarchy is built on the host\n");
        if (amg_device_setup and diffusivity_active()) rstdout("amg_device_setup: with a diffusivity set the low-order hierarchy is built on the host\n");
        if (amg_device_setup and is_composite) rstdout("amg_device_setup: a composite region builds its low-order hierarchy on the host\n");
        // the lattice the level-0 dofs sit on (the GLL points of the degree-N elements): the leading levels of the
        // hierarchy coarsen it geometrically (low_order.hpp); the device build also takes its point -> dof rows
        fdd::low_order::Lattice lattice;
        if ((options.geometric_levels or on_device) and poly_degree[0] >= 2)
        {
            const int n = poly_degree[0] + 1;
            lattice.dim = dim;
            lattice.n = n;
            lattice.ref.resize(n);
            std::vector<double> w(n);
            fdd::gll::zwgll(lattice.ref.data(), w.data(), n);
            if (is_composite)
                lattice.rows = fdd::composite::lattice_rows(comp, lattice.ref, (double)epsilon, lattice.num_elements);
            else
            {
                lattice.num_elements = fine_mesh->num_local_elements;
                const size_t np = (size_t)lattice.num_elements * n * n * n;
                fdd::low_order::HostCSR &R = lattice.rows;
                R.rows = (int)np;
                R.cols = num_dofs;
                R.ptr.assign(np + 1, 0);
                for (size_t q = 0; q < np; q++) R.ptr[q + 1] = R.ptr[q] + (point_dof[q] >= 0 ? 1 : 0);
                R.col.resize((size_t)R.ptr[np]);
                fdd::low_order::parallel_ranges((long long)np, fdd::low_order::range_parts((long long)np), [&](long long q0, long long q1, int) {
                    for (long long q = q0; q < q1; q++)
                        if (point_dof[q] >= 0) R.col[R.ptr[q]] = point_dof[q];
                });
                R.val.assign(R.col.size(), 1.0);
            }
        }
        options.lambda_max = [this](const fdd::low_order::HostCSR &M, const std::vector<double> &D, int iterations) { return device_lambda_max(M, D, iterations); };
        {
            // the run-time switches of the cycle belong to the problem, not to one hierarchy: a build (explicit, on first
            // use, or again) keeps what fddh_problem_set_flag stored
            const bool graph = amg_hierarchy.use_graph, fused = amg_hierarchy.fused_smoother, matrix_free = amg_hierarchy.matrix_free_transfer;
            const int bits = amg_hierarchy.precision;
            amg_hierarchy = amg::Hierarchy();
            amg_hierarchy.use_graph = graph;
            amg_hierarchy.fused_smoother = fused;
            amg_hierarchy.matrix_free_transfer = matrix_free;
            amg_hierarchy.precision = (bits == 32 and cheby_order >= 2) ? 32 : 64;
        }
        amg_hierarchy.cheby_order = cheby_order;
        amg_hierarchy.num_vcycles = num_vcycles;
        amg_levels_on_device = 0;
        amg_built_here = false;
        fdd::low_order::HostCSR A;
        int first_host_level = 0, geometric_done = 0;
        double t1 = 0.0;
        if (on_device)
        {
            namespace S = fdd::amg_setup;
            double t_mark = clock();
            auto lap = [&](const char *what, int l) {
                if (not(timing or verbose)) return;
                FDD_CALL(fdd_stream_sync(fdd::dev().stream));
                const double t = clock();
                if (timing or verbose) printf("low_order: device setup: level %d %-22s %7.3f s\n", l, what, t - t_mark);
                t_mark = t;
            };
            S::least_free() = (size_t)-1;
            S::note_memory();
            // the level-0 lattice in HBM: its point -> dof array (every later lattice is made from it on the device)
            S::DeviceLattice DL;
            DL.n = poly_degree[0] + 1;
            DL.cols = num_dofs;
            DL.ref = lattice.ref;
            DL.num_elements = fine_mesh->num_local_elements;
            DL.point_dof = fdd::dev().malloc<int>(std::max<size_t>(point_dof.size(), 1));
            DL.point_dof.copyFrom(point_dof.data(), point_dof.size() * sizeof(int));
            S::DeviceCSR Ad = S::assemble_fem(fine_mesh->x.data(), fine_mesh->y.data(), fine_mesh->z.data(), DL.point_dof, lattice.rows, num_dofs, poly_degree[0], fine_mesh->num_local_elements, epsilon);
            lap("FEM matrix", 0);
            t1 = clock();
            const bool use_lattice = options.geometric_levels;
            lattice = fdd::low_order::Lattice(); // the host's copy is not needed any more
            int l = 0;
            for (;; l++)
            {
                const int n = Ad.rows;
                const fdd::low_order::LevelPlan plan = fdd::low_order::plan_level(options, l, n, use_lattice ? DL.host(false) : fdd::low_order::Lattice(), geometric_done);
                if (not plan.geometric) break; // hand-off: this level and the ones below it are built on the host
                fdd::memory D = S::inv_sqrt_diag(Ad);
                const double lmax = device_lambda_max(n, Ad.ptr_hst, Ad.ptr, Ad.col, Ad.val, D, options.power_iterations);
                fdd::low_order::Options ol = options;
                ol.eig_ratio = plan.eig_ratio;
                const std::vector<double> coefs = fdd::low_order::chebyshev_coefficients(lmax, ol);
                if (verbose) printf("low_order: level %d rows %d nnz %lld lambda_max(DAD) %.4f\n", l, n, Ad.nnz(), lmax);
                lap("diagonal + lambda_max", l);
                geometric_done++;
                S::DeviceLattice next;
                fdd::low_order::Transfer transfer;
                S::DeviceCSR Pd = S::geometric_level(DL, n, next, transfer);
                DL = std::move(next);
                if (verbose) printf("low_order: level %d coarsened on the lattice: %d -> %d rows, %d nodes per direction and element left\n", l, n, Pd.cols, DL.n);
                lap("interpolator", l);
                S::DeviceCSR Rd = S::transpose(Pd);                   // low_order::transpose, for the Galerkin product
                S::DeviceCSR Rv = S::transpose(Pd, 1.0e-12);          // CSR_Matrix::transpose, the V-cycle's R
                lap("transpose", l);
                S::DeviceCSR AP = S::multiply(Ad, Pd);
                lap("A P", l);
                S::DeviceCSR Ac = S::multiply(Rd, AP);
                lap("R (A P)", l);
                AP.free();
                Rd.free();
                const int nc = Pd.cols;
                amg_hierarchy.add_level_device(n, std::move(Ad.ptr_hst), Ad.ptr, Ad.col, Ad.val, D, coefs.data(), nc, std::move(Pd.ptr_hst), Pd.ptr, Pd.col, Pd.val, std::move(Rv.ptr_hst), Rv.ptr, Rv.col, Rv.val);
                amg_hierarchy.set_lattice_transfer((size_t)l, std::move(transfer));
                lap("level attached", l);
                Ad = Ac;
            }
            A = S::download(Ad);
            if (use_lattice) lattice = DL.host(true); // small by now (C2 / C3: the degree-1 lattice)
            lap("hand-off download", l);
            S::note_memory();
            if (timing)
            {
                size_t free_b = 0, total_b = 0;
                FDD_CALL(fdd_amg_setup_memory_info(&free_b, &total_b));
                printf("low_order: device setup: peak device memory in use %.2f GB of %.2f GB (sampled after each allocation step)\n", (double)(total_b - S::least_free()) / 1e9, (double)total_b / 1e9);
            }
            first_host_level = l;
            amg_levels_on_device = l + 1; // the matrices of levels 0 .. l (level l's is the device loop's last Galerkin product)
        }
        else
        {
            if (is_composite)
            {
                // the composite's low-order operator: mixed-degree region with its hanging edges / faces, plus the
                // superdomain rows (subdomain.tpp:2749-3472, composite.hpp)
                std::vector<std::vector<double>> nodes(num_levels);
                for (int l = 0; l < num_levels; l++)
                {
                    const int n = poly_degree[l] + 1;
                    std::vector<double> w(n);
                    nodes[l].resize(n);
                    fdd::gll::zwgll(nodes[l].data(), w.data(), n);
                }
                A = fdd::composite::assemble_low_order(comp, nodes, D_hat[num_levels - 1].first, (double)epsilon);
            }
            else
            {
                A = fdd::low_order::assemble_fem(fine_mesh->x.data(), fine_mesh->y.data(), fine_mesh->z.data(), point_dof.data(), num_dofs, poly_degree[0], fine_mesh->num_local_elements, epsilon, diffusivity_active() ? diffusivity_hst.data() : nullptr);
                // the Helmholtz term on the diagonal of the level-0 matrix: the coarse operators are Galerkin products of it
                for (int d = 0; d < std::min((int)shift_dofs_hst.size(), A.rows); d++)
                    for (int t = A.ptr[d]; t < A.ptr[d + 1]; t++)
                        if (A.col[t] == d) A.val[t] += shift_dofs_hst[d];
            }
            t1 = clock();
        }
        std::vector<fdd::low_order::Level> lv = fdd::low_order::build(std::move(A), options, verbose, std::move(lattice), first_host_level, geometric_done);
        const double t2 = clock();
        for (size_t l = 0; l < lv.size(); l++)
        {
            const bool coarsest = (l + 1 == lv.size());
            fdd::low_order::Level &L = lv[l];
            if (coarsest) L.P = fdd::low_order::HostCSR();
            const int n = L.A.rows, nc = L.P.cols;
            amg_hierarchy.add_level_adopt(n, std::move(L.A.ptr), std::move(L.A.col), std::move(L.A.val), L.D.data(), L.coefs.data(), nc, std::move(L.P.ptr), std::move(L.P.col), std::move(L.P.val));
            amg_hierarchy.set_lattice_transfer((size_t)first_host_level + l, std::move(L.transfer)); // a geometric level: its interpolator is applied matrix-free
            lv[l] = fdd::low_order::Level(); // free the host copy as we go
        }
        if (verbose) printf("low_order: FEM matrix %.2f s, hierarchy %.2f s, levels to the device %.2f s (%d host threads)\n", t1 - t0, t2 - t1, clock() - t2, fdd::low_order::host_threads());
        amg_finalize();
        amg_built_here = true;
        amg_setup_seconds = clock() - t0;
        if (timing) printf("low_order: AMG setup %.3f s, %d of %d levels built on the device\n", amg_setup_seconds, amg_levels_on_device, (int)amg_hierarchy.levels.size());
        return (int)amg_hierarchy.levels.size();
    }
    // the hierarchy in place is amg_build's own (not handed in through amg_add_level): it can be made again
    bool amg_built_here = false;
    fdd::low_order::Options amg_build_options;
    void amg_rebuild() { rebuild_own_hierarchy(("amg_cheby_order " + std::to_string(cheby_order)).c_str()); }
    bool amg_device_setup = false; // "amg_device_setup": amg_build makes the FEM matrix and the lattice levels in HBM (conforming regions)
    int amg_levels_on_device = 0;  // of the last amg_build: the levels whose matrix A was computed on the device
    double amg_setup_seconds = 0.0;
    void apply_low_order_preconditioner(fdd::memory &z, fdd::memory &r) { low_order_preconditioner(z, r); }

    bool block_local = false;             // more than one rank: keep the rank's own elements only (no rings, no superdomain): block-Jacobi, the comparison point
    bool force_composite = false;         // build the region through composite.hpp even on one rank (test hook: must equal the conforming region)
    bool composite() const { return is_composite; }
    const fdd::composite::Composite &composite_description() const { return comp; }
    fdd::composite::GradingOptions grading; // superdomain coarsening (composite.hpp)
    bool build_tree = true;               // run the degree-tree restrictions as the reference always does
    bool fused_dssum = true;              // gather-scatter kernel instead of the Qt / QQt_int / Q SpMV chain
    bool restructured = true;             // inner GMRES with cached assembled basis, multi-dot / multi-axpy
    bool assembled_inner = true;          // inner GMRES on vectors over the dofs: Q fused into the stiffness load, no point-space Krylov basis
    bool device_bookkeeping = true;       // assembled inner GMRES: Givens / stopping tests in one-thread kernels, one host sync per cycle
    bool unit_norm_weight() const { return norm_weight_is_one; }
    bool fold_coarse_exchange = true;     // the coarse level's blocks travel inside the ring pull's group (false: an all-gather of their own)
    bool skip_last_basis_store = true;    // device GMRES: the last Arnoldi step of a cycle forms the norm of its vector without storing it (nobody reads it)
    // dof-space GMRES in double, m < FDD_MULTI_MAX: the last Arnoldi step of a cycle takes |q - sum h v|^2 from <q, q> and the
    // projections where include/fdd_norm_estimate.h allows it, and the exact pass runs (gated on the device, no host in between)
    // only where it does not.  Changes rounding, not more: DESIGN section 4.3.  On where the kernel library has the entries; at 0
    // every launch is the one it was.  Which norm the step takes depends on this flag alone, not on skip_last_basis_store.
    bool last_norm_from_projections = fdd::missing_norm_estimate_entry() == nullptr;
    bool norm_from_projections_at(int j) const { return last_norm_from_projections and precision != 32 and j + 1 == num_vectors and num_vectors < FDD_MULTI_MAX; }
    long long host_norm_estimated = 0, host_norm_exact = 0; // the host-bookkeeping loop's share of the counters below
    double host_min_ratio = 0.0;
    // over the life of this Subdomain: the last steps that took the estimate, those that fell back to the exact pass, and the
    // smallest est / <q, q> among them (0 before the first); one blocking read of the device state
    void norm_counters(long long &estimated, long long &exact, double &min_ratio)
    {
        estimated = host_norm_estimated, exact = host_norm_exact, min_ratio = host_min_ratio;
        if (not gmres_state.ptr() or fdd::missing_norm_estimate_entry() != nullptr) return;
        long long e = 0, x = 0;
        double r = 0.0;
        FDD_CALL(fdd_gmres_fetch_norm_counters(gmres_state.ptr(), &e, &x, &r, fdd::dev().stream));
        if (e + x > 0 and (estimated + exact == 0 or r < min_ratio)) min_ratio = r;
        estimated += e, exact += x;
    }
    bool history_pending = false;         // the last solve ran with InnerSolveHints::lazy_history and its history is still on the device

    // residual_history of the last lazy solve (one blocking read of the device state)
    void finish_history()
    {
        if (not history_pending or not gmres_state.ptr()) return;
        std::vector<double> hist(FDD_MULTI_MAX + 1);
        int nh = 0, j_last = -1, steps = 0, converged = 0;
        FDD_CALL(fdd_gmres_fetch(gmres_state.ptr(), nullptr, hist.data(), &nh, &j_last, &steps, &converged, fdd::dev().stream));
        residual_history.assign(hist.begin(), hist.begin() + nh);
        history_pending = false;
    }
    fdd::StiffnessFlags stiffness; // which kernel each element list runs (element_operator.hpp)
    std::vector<DType> residual_history;  // inner history of the last application

    int num_values = 0;
    std::vector<int> point_dof; // dof of every level-0 subdomain point, -1 on Dirichlet points (the rows of Q)

    Subdomain() {}

    // subdomain.tpp:86-...: `domains` maps polynomial degree -> Domain of this rank
    template <typename PType>
    Subdomain(std::unordered_map<int, PType> &domains, int poly_degree_, int poly_reduction_, int subdomain_overlap_ = 1, int superdomain_overlap_ = 1)
    {
        initialize(domains, poly_degree_, poly_reduction_, subdomain_overlap_, superdomain_overlap_);
    }

    int levels_count() const { return num_levels; }
    const std::vector<int> &level_degrees() const { return poly_degree; }
    int dofs() const { return num_dofs; }

    template <typename PType>
    void initialize(std::unordered_map<int, PType> &domains, int poly_degree_, int poly_reduction_, int subdomain_overlap_ = 1, int superdomain_overlap_ = 1)
    {
        PType &domain = domains[poly_degree_];
        dim = domain.mesh.dim;
        fine_mesh = &domain.mesh;

        poly_reduction = poly_reduction_;
        subdomain_overlap = subdomain_overlap_;
        superdomain_overlap = superdomain_overlap_;

        // levels N, N-r, ..., 1 (subdomain.tpp:98-110)
        poly_degree.clear();
        poly_degree.push_back(poly_degree_);
        while (poly_degree.back() > 1)
        {
            int reduced = poly_degree.back() - poly_reduction;
            poly_degree.push_back(reduced >= 1 ? reduced : 1);
        }
        num_levels = (int)poly_degree.size();

        levels.resize(num_levels);
        for (int l = 0; l < num_levels; l++)
        {
            PType &dl = domains[poly_degree[l]];
            levels[l].num_points = dl.num_local_points;
            levels[l].num_elements = dl.num_local_elements;
            levels[l].poly_degree = dl.poly_degree;
            levels[l].offset = (l > 0) ? levels[l - 1].offset + levels[l - 1].num_points : 0;
        }

        // interpolators between every pair of levels (subdomain.tpp:142-164)
        for (int l_f = 0; l_f < num_levels - 1; l_f++)
            for (int l_c = l_f + 1; l_c < num_levels; l_c++)
            {
                std::pair<int, int> idx(poly_degree[l_c], poly_degree[l_f]);
                if (J_cf.count(idx)) continue;
                auto &entry = J_cf[idx];
                entry.first = fdd::gll::interpolator(poly_degree[l_c], poly_degree[l_f]);
                entry.second = fdd::dev().malloc<DType>(entry.first.size());
                entry.second.copyFrom(entry.first.data(), entry.first.size() * sizeof(DType));
            }

        // reference operators per level (subdomain.tpp:166-196): the Domains' own tables
        D_hat.resize(num_levels);
        for (int l = 0; l < num_levels; l++)
        {
            PType &dl = domains[poly_degree[l]];
            D_hat[l].first = dl.D_hat_hst;
            D_hat[l].second = dl.D_hat;
        }

        is_composite = (fdd::comm().size > 1 and not block_local) or force_composite;
        if (is_composite)
            initialize_composite(domains, domain);
        else
            initialize_conforming(domains, domain);

        num_values = subdomain_operator.num_points + superdomain_operator.num_extended_dofs; // subdomain.tpp:3858
        num_blocks = (num_values + BLOCK_SIZE - 1) / BLOCK_SIZE;

        {
            inner_weight = fdd::dev().malloc<DType>(num_values);
            subdomain_operator.Q.multiply(inner_weight, norm_weight);
            std::vector<DType> w(num_values);
            inner_weight.copyTo(w.data(), (size_t)num_values * sizeof(DType));
            // the tail takes the superdomain part of norm_weight (subdomain.tpp:2742-2744)
            for (int i = 0; i < superdomain_operator.num_extended_dofs; i++) w[(size_t)subdomain_operator.num_points + i] = norm_weight_hst[(size_t)subdomain_operator.num_extended_dofs + i];
            for (int i = 0; i < num_values; i++)
                if (w[i] > 0.0) w[i] = 1.0;
            inner_weight.copyFrom(w.data(), (size_t)num_values * sizeof(DType));
        }

        // solver vectors (subdomain.tpp:3860-3873)
        f = fdd::dev().malloc<DType>(num_values);
        u_k = fdd::dev().malloc<DType>(num_values);
        r_k = fdd::dev().malloc<DType>(num_values);
        r_kp1 = fdd::dev().malloc<DType>(num_values);
        q_k = fdd::dev().malloc<DType>(num_values);
        z_k = fdd::dev().malloc<DType>(num_values);
        p_k = fdd::dev().malloc<DType>(num_values);
        // (the point-space Krylov basis is allocated by the solvers that use it)

        reduce_ws = fdd::dev().malloc<double>(fdd_reduce_workspace_doubles());
        scalars = fdd::dev().malloc<double>(2 * FDD_GMRES_SLOT);

        // the big boolean matrices' host mirrors are not needed after setup
        subdomain_operator.Q.release_host();
        subdomain_operator.Qt.release_host();
    }

    // the region of a single rank (or of a block-local run): the rank's own conforming elements
    template <typename PType>
    void initialize_conforming(std::unordered_map<int, PType> &domains, PType &domain)
    {
        const int P = domain.num_local_points;
        const int total_level_points = levels[num_levels - 1].offset + levels[num_levels - 1].num_points;

        // work arrays hold the whole degree tree (subdomain.tpp:588-595)
        work_dev.resize(3);
        for (int w = 0; w < 3; w++) work_dev[w] = fdd::dev().malloc<DType>((size_t)total_level_points + (size_t)P + 16);

        // region geometry = own fine-level data (subdomain.tpp:667-699)
        for (int g = 0; g < NUM_GEOM_FACTS; g++) subdomain_operator.geom_fact[g] = domain.geom_fact[g];

        // dof numbering.  The reference ranks the global ids of the unmasked points
        // (subdomain.tpp:1151-1176); every numbering of those nodes gives the same
        // operators, and nothing outside the class sees it except the AMG hierarchy,
        // which is handed in against sub_point_dofs.  Here the dofs follow the
        // Domain's node order with the masked nodes dropped, so that moving between
        // Domain node vectors and subdomain dof vectors (Domain::precondition_nodes)
        // is a monotone compaction instead of a scattered permutation.
        std::vector<double> tmp(P);
        {
            const auto &node = domain.scatter_matrix().col_hst; // one entry per point
            std::vector<int> dof_of_node(domain.num_local_nodes, 0);
            for (int p = 0; p < P; p++)
                if (domain.mesh.p_mask[p] > 0.0) dof_of_node[node[p]] = 1;
            int count = 0;
            for (int n = 0; n < domain.num_local_nodes; n++)
                if (dof_of_node[n]) dof_of_node[n] = ++count;
            for (int p = 0; p < P; p++) tmp[p] = (domain.mesh.p_mask[p] > 0.0) ? (double)dof_of_node[node[p]] : 0.0;
        }

        int max_dof = 0;
        for (int p = 0; p < P; p++) max_dof = std::max(max_dof, (int)tmp[p]);

        // Q (subdomain.tpp:1510-1520, 1584)
        {
            // at most one unit entry per point, rows in order: what add_entry + assemble produce, written directly
            std::vector<int> q_ptr((size_t)P + 1, 0);
            for (int p = 0; p < P; p++) q_ptr[p + 1] = q_ptr[p] + (tmp[p] > 0.0 ? 1 : 0);
            fdd::low_order::pod_vector<int> q_col((size_t)q_ptr[P]);
            fdd::low_order::pod_vector<DType> q_val((size_t)q_ptr[P]);
            fdd::low_order::parallel_ranges(P, fdd::low_order::range_parts(P), [&](long long p0, long long p1, int) {
                for (long long p = p0; p < p1; p++)
                    if (tmp[p] > 0.0)
                    {
                        q_col[q_ptr[p]] = (int)tmp[p] - 1;
                        q_val[q_ptr[p]] = (DType)1.0;
                    }
            });
            if (q_ptr[P] > 0)
                subdomain_operator.Q.adopt_csr(P, max_dof, std::move(q_ptr), std::move(q_col), std::move(q_val));
            else
                subdomain_operator.Q.initialize(P, max_dof);
        }
        subdomain_operator.Q.transpose(subdomain_operator.Qt);
        assembly.clear(); // the classes of another Qt
        point_dof.assign(P, -1);
        for (int p = 0; p < P; p++)
            if (tmp[p] > 0.0) point_dof[p] = (int)tmp[p] - 1;
        point_dof_dev = fdd::dev().malloc<int>(std::max(P, 1));
        point_dof_dev.copyFrom(point_dof.data(), (size_t)P * sizeof(int));
        {
            std::vector<int> no_dof;
            for (int p = 0; p < P; p++)
                if (!(tmp[p] > 0.0)) no_dof.push_back(p);
            num_points_without_dof = (int)no_dof.size();
            points_without_dof = fdd::dev().malloc<int>(std::max(num_points_without_dof, 1));
            points_without_dof.copyFrom(no_dof.data(), no_dof.size() * sizeof(int));
        }
        std::vector<double>().swap(tmp);

        subdomain_operator.num_dofs = max_dof;
        subdomain_operator.num_points = subdomain_operator.Q.num_rows;
        subdomain_operator.num_extended_dofs = subdomain_operator.Q.num_cols;

        // one contiguous level-0 element list (subdomain.tpp:1603-1630 sorted by level)
        {
            fdd::LevelList ll;
            ll.level = 0;
            ll.poly_degree = poly_degree[0];
            ll.dim = dim;
            ll.D_hat = D_hat[0].second.template as<double>();
            ll.num_elements = domain.num_local_elements;
            ll.first_offset = 0;
            for (int g = 0; g < NUM_GEOM_FACTS; g++) ll.G[g] = subdomain_operator.geom_fact[g].template as<double>();
            fdd::detect_zero_factors(ll);
            fdd::detect_shared_blocks(ll);
            fdd::check_lean_table(ll, D_hat[ll.level].first);
            subdomain_operator.level_lists.push_back(ll);
        }

        // superdomain: empty
        superdomain_operator.num_dofs = 0;
        superdomain_operator.num_points = 0;
        superdomain_operator.num_extended_dofs = 0;

        // Qt_coarse (subdomain.tpp:1653-1713) on this rank's coarsest-level elements
        {
            PType &coarse = domains[poly_degree[num_levels - 1]];
            const int size = coarse.num_local_points;
            std::vector<double> dof(size);
            for (int i = 0; i < size; i++) dof[i] = (coarse.mesh.p_mask[i] > 0.0) ? (double)coarse.mesh.glo_num[i] : 0.0;
            ranking(dof);
            int num_coarse_dofs = 0;
            for (int i = 0; i < size; i++) num_coarse_dofs = std::max(num_coarse_dofs, (int)dof[i]);
            Qt_coarse.initialize(num_coarse_dofs, size);
            Qt_coarse.reserve(size);
            for (int i = 0; i < size; i++)
                if (dof[i] > 0.0) Qt_coarse.add_entry((int)dof[i] - 1, i, 1.0);
            Qt_coarse.assemble();
        }

        // interface operators (subdomain.tpp:2581-2729) reduce to identities
        num_interface_dofs = 0;
        num_dofs = subdomain_operator.num_dofs + superdomain_operator.num_dofs - num_interface_dofs;
        identity_matrix(Q_int, num_dofs);
        identity_matrix(Qt_int, num_dofs);
        identity_matrix(QQt_int, num_dofs);

        // weights (subdomain.tpp:2731-2747)
        {
            const int nw = subdomain_operator.num_extended_dofs + superdomain_operator.num_extended_dofs;
            std::vector<DType> w(std::max(nw, 1), 1.0);
            norm_weight = fdd::dev().malloc<DType>(std::max(nw, 1));
            norm_weight.copyFrom(w.data(), w.size() * sizeof(DType));
            norm_weight_hst = w;
            norm_weight_is_one = true; // no interface dofs shared with a superdomain: the kernels need not read it
        }

    }

    // one unit entry per row (or none where col < 0): the interface maps of subdomain.tpp:2653-2729
    static void unit_matrix(CSR_Matrix<DType> &A, int rows, int cols, const int *col)
    {
        std::vector<int> ptr(rows + 1, 0), cc;
        std::vector<DType> vv;
        for (int i = 0; i < rows; i++)
        {
            if (col[i] >= 0)
            {
                cc.push_back(col[i]);
                vv.push_back(1.0);
            }
            ptr[i + 1] = (int)cc.size();
        }
        A.assemble_from_csr(rows, cols, ptr.data(), cc.data(), vv.data());
    }

    static void host_csr_matrix(CSR_Matrix<DType> &A, const fdd::low_order::HostCSR &H)
    {
        A.assemble_from_csr(H.rows, H.cols, H.ptr.data(), H.col.data(), H.val.data());
    }

    // the composite region of a multi-rank run (subdomain.tpp:198-2747 via composite.hpp), uploaded
    template <typename PType>
    void initialize_composite(std::unordered_map<int, PType> &domains, PType &domain)
    {
        fdd::SetupTimer setup_timing("Subdomain::initialize_composite", fdd::comm().rank == 0);
        std::map<std::pair<int, int>, std::vector<double>> J;
        for (auto &kv : J_cf) J[kv.first] = kv.second.first;
        comp = fdd::composite::build(domains, poly_degree, subdomain_overlap, superdomain_overlap, (double)epsilon, J, D_hat[num_levels - 1].first, std::vector<int>(domain.scatter_matrix().col_hst.begin(), domain.scatter_matrix().col_hst.end()), domain.num_local_nodes, grading);
        setup_timing.lap("composite::build");
        const fdd::composite::Composite &c = comp;

        own_points = levels[0].num_points;
        const int NP = c.num_sub_ext_points;
        const int nse = c.sub_num_ext_dofs, nue = c.sup_num_ext_dofs;
        num_ring_points = NP - own_points;

        rstdout("Composite region: %d own + %d ring + %d extended elements (%d points), %d + %d subdomain dofs, %d interface, superdomain %d of %d coarse dofs (+%d extended), %d unique dofs\n", levels[0].num_elements,
                c.num_sub_elems - levels[0].num_elements, c.num_sub_ext_elems - c.num_sub_elems, NP, c.sub_num_dofs, nse - c.sub_num_dofs, c.num_interface_dofs, c.sup_num_dofs, c.num_coarse_dofs, nue - c.sup_num_dofs, c.num_dofs);

        // geometry (subdomain.tpp:667-699).  With ring elements the region gets its own factor arrays over ALL its
        // points, own elements included (a copy of the Domain's: 48 B per own point), so that the degree-N ring is
        // one element list with the own elements -- one launch per polynomial level; two lists would cost a second,
        // latency-bound launch of ~1000 elements in every operator application.  Without rings (a one-rank composite)
        // the Domain's arrays serve.
        const bool own_copy = num_ring_points > 0;
        for (int g = 0; g < NUM_GEOM_FACTS; g++)
        {
            if (own_copy)
            {
                ring_geom[g] = fdd::dev().malloc<DType>(std::max(NP, 1));
                ring_geom[g].copyFrom(c.G[g].data(), (size_t)NP * sizeof(DType));
                subdomain_operator.geom_fact[g] = ring_geom[g];
            }
            else
                subdomain_operator.geom_fact[g] = domain.geom_fact[g];
        }

        setup_timing.lap("region geometry to the device");
        // level-sorted element lists (subdomain.tpp:1603-1630 sorted by level): the region is ordered by level, so
        // every degree is one contiguous run of elements
        subdomain_operator.level_lists.clear();
        for (int l = 0; l < num_levels; l++)
        {
            const int first = c.level_first_elem[l], count = c.level_num_elems[l];
            if (count == 0) continue;
            fdd::LevelList ll;
            ll.level = l;
            ll.poly_degree = poly_degree[l];
            ll.dim = dim;
            ll.D_hat = D_hat[l].second.template as<double>();
            ll.num_elements = count;
            ll.first_offset = c.sub[first].offset;
            for (int g = 0; g < NUM_GEOM_FACTS; g++) ll.G[g] = subdomain_operator.geom_fact[g].template as<double>() + ll.first_offset;
            fdd::detect_zero_factors(ll); // own elements and every ring's run, each on its own
            fdd::detect_shared_blocks(ll);
            fdd::check_lean_table(ll, D_hat[ll.level].first);
            subdomain_operator.level_lists.push_back(ll);
        }

        // Q with its J_cf rows, Qt (subdomain.tpp:1496-1585)
        subdomain_operator.Q.initialize(NP, nse);
        subdomain_operator.Q.reserve(c.Q_row.size());
        for (size_t t = 0; t < c.Q_row.size(); t++) subdomain_operator.Q.add_entry(c.Q_row[t], c.Q_col[t], c.Q_val[t]);
        subdomain_operator.Q.assemble();
        subdomain_operator.Q.transpose(subdomain_operator.Qt);
        assembly.clear(); // the classes of another Qt
        subdomain_operator.num_dofs = c.sub_num_dofs;
        subdomain_operator.num_points = NP;
        subdomain_operator.num_extended_dofs = nse;

        setup_timing.lap("Q and Qt");
        point_dof = c.point_dof;
        point_dof_dev = fdd::dev().malloc<int>(std::max(NP, 1));
        point_dof_dev.copyFrom(point_dof.data(), (size_t)NP * sizeof(int));

        // superdomain operator (subdomain.tpp:2541-2575) and the coarse assembly (:1706-1713).  The coarse level is
        // all-gathered with a fixed count per rank, so Qt_coarse's columns address that padded layout.
        superdomain_operator.num_dofs = c.sup_num_dofs;
        superdomain_operator.num_extended_dofs = nue;
        superdomain_operator.num_points = 0;
        host_csr_matrix(superdomain_operator.A, c.A_sup);
        host_csr_matrix(superdomain_operator.Pt, c.Pt_sup);
        {
            const int nv = c.num_vertices, R = fdd::comm().size;
            int max_count = 0;
            for (int p = 0; p < R; p++) max_count = std::max(max_count, c.proc_count[p]);
            coarse_pad = max_count * nv;
            std::vector<int> owner_of(c.num_total_elements);
            for (int p = 0; p < R; p++)
                for (int e = 0; e < c.proc_count[p]; e++) owner_of[c.proc_offset[p] + e] = p;
            fdd::low_order::HostCSR Q = c.Qt_coarse;
            for (int &col : Q.col)
            {
                const int e = col / nv, v = col % nv, p = owner_of[e];
                col = p * coarse_pad + (e - c.proc_offset[p]) * nv + v;
            }
            Q.cols = R * coarse_pad;
            // the remap is monotone inside a rank and ranks are in order: rows stay sorted
            host_csr_matrix(Qt_coarse, Q);
            coarse_all = fdd::dev().malloc<DType>(std::max((size_t)R * coarse_pad, (size_t)1));
        }

        setup_timing.lap("superdomain operators");
        // interface maps and weights (subdomain.tpp:2581-2747)
        num_interface_dofs = c.num_interface_dofs;
        num_dofs = c.num_dofs;
        unit_matrix(Q_int, nse + nue, num_dofs, c.Q_int_col.data());
        unit_matrix(Qt_int, num_dofs, nse + nue, c.Qt_int_col.data());
        unit_matrix(QQt_int, nse + nue, nse + nue, c.QQt_int_col.data());
        norm_weight_hst.assign(c.norm_weight.begin(), c.norm_weight.end());
        norm_weight = fdd::dev().malloc<DType>(std::max(nse + nue, 1));
        norm_weight.copyFrom(norm_weight_hst.data(), norm_weight_hst.size() * sizeof(DType));
        norm_weight_is_one = false;

        setup_timing.lap("interface maps and weights");
        // solve-time ring pull: what this rank packs for its peers and where the answers land
        {
            std::vector<int> sidx, uidx((size_t)std::max(num_ring_points, 1), 0);
            size_t recv_total = 0;
            for (const fdd::composite::PeerPlan &pl : c.peers) recv_total += (size_t)pl.recv_points;
            exchange_ops.clear();
            std::vector<size_t> send_at, recv_at;
            size_t rat = 0;
            for (const fdd::composite::PeerPlan &pl : c.peers)
            {
                send_at.push_back(sidx.size());
                recv_at.push_back(rat);
                for (size_t k = 0; k < pl.send_level.size(); k++)
                {
                    const int l = pl.send_level[k], e = pl.send_elem[k];
                    const int np = levels[l].num_points / std::max(levels[l].num_elements, 1);
                    for (int v = 0; v < np; v++) sidx.push_back(levels[l].offset + e * np + v);
                }
                for (int r : pl.recv_elem)
                    for (int v = 0; v < c.sub[r].num_points; v++) uidx[(size_t)c.sub[r].offset - own_points + v] = (int)rat++;
            }
            num_send_points = (int)sidx.size();
            send_index = fdd::dev().malloc<int>(std::max(num_send_points, 1));
            send_index.copyFrom(sidx.data(), sidx.size() * sizeof(int));
            send_all = fdd::dev().malloc<DType>(std::max(num_send_points, 1));
            recv_all = fdd::dev().malloc<DType>(std::max(recv_total, (size_t)1));
            unpack_index = fdd::dev().malloc<int>(std::max(num_ring_points, 1));
            unpack_index.copyFrom(uidx.data(), (size_t)num_ring_points * sizeof(int));
            for (size_t k = 0; k < c.peers.size(); k++)
            {
                fdd::ExchangeOp op;
                op.peer = c.peers[k].rank;
                op.send = send_all.template as<DType>() + send_at[k];
                op.send_bytes = (size_t)c.peers[k].send_points * sizeof(DType);
                op.recv = recv_all.template as<DType>() + recv_at[k];
                op.recv_bytes = (size_t)c.peers[k].recv_points * sizeof(DType);
                exchange_ops.push_back(op);
            }
        }

        // work arrays: the degree tree (plus the padded coarse send), region vectors, dof vectors, the gathered coarse level
        {
            const size_t total_level_points = (size_t)levels[num_levels - 1].offset + (size_t)levels[num_levels - 1].num_points;
            size_t W = std::max({total_level_points + (size_t)coarse_pad, (size_t)NP, (size_t)(nse + nue), (size_t)c.num_coarse_dofs, (size_t)num_dofs}) + 16;
            work_dev.resize(3);
            for (int w = 0; w < 3; w++) work_dev[w] = fdd::dev().malloc<DType>(W);
        }
        // the ring pull's ops followed by one op per other rank for the coarse blocks (both sides list them in this order)
        {
            exchange_ops_folded = exchange_ops;
            const int R = fdd::comm().size, me = fdd::comm().rank;
            DType *coarse = work_dev[0].template as<DType>() + levels[num_levels - 1].offset;
            for (int r = 0; r < R and coarse_pad > 0; r++)
            {
                if (r == me) continue;
                fdd::ExchangeOp op;
                op.peer = r;
                op.send = coarse;
                op.recv = coarse_all.template as<DType>() + (size_t)r * coarse_pad;
                op.send_bytes = op.recv_bytes = (size_t)coarse_pad * sizeof(DType);
                exchange_ops_folded.push_back(op);
            }
        }

        setup_timing.lap("exchange plan, work arrays");
        setup_composite_dofs();

        setup_timing.lap("setup_composite_dofs");
        // the per-point arrays the solve path no longer needs
        for (int g = 0; g < NUM_GEOM_FACTS; g++) std::vector<double>().swap(comp.G[g]);
        std::vector<int>().swap(comp.Q_row);
        std::vector<int>().swap(comp.Q_col);
        std::vector<double>().swap(comp.Q_val);
    }

    void allocate_krylov()
    {
        V.resize(num_vectors + 1);
        for (int i = 0; i < num_vectors + 1; i++) V[i] = fdd::dev().malloc<DType>(num_values);
        Z.resize(num_vectors);
        for (int i = 0; i < num_vectors; i++) Z[i] = fdd::dev().malloc<DType>(num_values);
    }

    // The inner iteration is the reference's Subdomain loop: gmres.hpp says what the two switches stand for.
    fdd::GmresControl<DType> inner_gmres_control(bool use_relative) const { return {max_iterations, tolerance, use_relative, /* count_at_step_start */ true, /* stop_on_nan */ false}; }
    static auto print_inner_step(bool print_history)
    {
        return [print_history](int step, DType r_norm, DType relative) {
            if (print_history) pstdout("- Iter %3d: | residual_norm = %24.16g | relative_residual_norm = %24.16g | \n", step, r_norm, relative);
        };
    }

    // subdomain.tpp:3969-3985
    void direct_stiffness_summation(fdd::memory &QQtu, fdd::memory &u)
    {
        if (fused_dssum and not is_composite and subdomain_operator.Qt.unit_values and QQt_int.is_identity and superdomain_operator.num_extended_dofs == 0)
        {
            // Q * I * Qt in one gather-scatter pass over the dofs; points without
            // a dof (Dirichlet: empty rows of Q) get the 0.0 the SpMV writes.
            subdomain_operator.Qt.gather_scatter(QQtu.as<double>(), nullptr, u.as<double>(), nullptr, nullptr, 0, subdomain_operator.num_extended_dofs, 0);
            FDD_CALL(fdd_fill_indexed(QQtu.as<double>(), points_without_dof.template as<int>(), 0.0, num_points_without_dof, fdd::dev().stream));
            return;
        }

        fdd::memory u_sub_l = u.slice(0, subdomain_operator.num_points);
        subdomain_operator.Qt.multiply(work_dev[0], u_sub_l);
        copy_tail(work_dev[0], u); // :3977
        QQt_int.multiply(work_dev[1], work_dev[0]);
        fdd::memory QQtu_sub_l = QQtu.slice(0, subdomain_operator.num_points);
        subdomain_operator.Q.multiply(QQtu_sub_l, work_dev[1]);
        copy_tail_back(QQtu, work_dev[1]); // :3984
    }

    // subdomain.tpp:3942-3967
    void stiffness_matrix(fdd::memory &Au, fdd::memory &u)
    {
        fdd::memory u_sub_l = u.slice(0, subdomain_operator.num_points);
        fdd::memory u_sup = u.slice(subdomain_operator.num_points, superdomain_operator.num_extended_dofs);
        fdd::memory Au_sub_l = Au.slice(0, subdomain_operator.num_points);
        fdd::memory Au_sup = Au.slice(subdomain_operator.num_points, superdomain_operator.num_extended_dofs);

        superdomain_operator.A.multiply(Au_sup, u_sup); // empty: no-op

        for (auto &ll : subdomain_operator.level_lists) fdd::apply_local(ll, Au_sub_l.as<double>(), u_sub_l.as<double>(), work_dev, stiffness);
    }

    // subdomain.tpp:4161-4268
    void flexible_conjugate_gradient(fdd::memory &u_l, fdd::memory &f_l, bool print_history = true, bool use_relative = false)
    {
        if (inner_solver == 1) return generalized_minimum_residual(u_l, f_l, print_history, use_relative); // Chebyshev-Jacobi takes the place of either Krylov solve
        begin_inner_solve();
        tree_operator(r_k, f_l);

        fdd_timer().start("subdomain.vector_operations");
        math.set_to_value(u_k, 0.0, num_values);
        fdd_timer().stop("subdomain.vector_operations");

        DType r_norm;
        DType r_0_norm;

        fdd_timer().start("subdomain.residual_norm");
        residual_norm(r_0_norm, r_k);
        fdd_timer().stop("subdomain.residual_norm");
        residual_history.push_back(r_0_norm);
        if (print_history) pstdout("- Iter %3d: | residual_norm = %24.16g | relative_residual_norm = %24.16g | \n", 0, r_0_norm, 1.0);

        DType alpha_k, beta_k, gamma_k, theta_k;

        fdd_timer().start("subdomain.preconditioner");
        if (use_preconditioner)
            low_order_preconditioner(z_k, r_k);
        else if (use_jacobi)
            jacobi_preconditioner(z_k, r_k);
        else
            direct_stiffness_summation(z_k, r_k);
        fdd_timer().stop("subdomain.preconditioner");

        fdd_timer().start("subdomain.vector_operations");
        p_k.copyFrom(z_k, (size_t)num_values * sizeof(DType));
        fdd_timer().stop("subdomain.vector_operations");

        int iter = 0;

        while (iter < max_iterations)
        {
            fdd_timer().start("subdomain.operator_application");
            stiffness_matrix(q_k, p_k);
            fdd_timer().stop("subdomain.operator_application");

            fdd_timer().start("subdomain.inner_products");
            projection_inner_products(gamma_k, theta_k, z_k, r_k, p_k, q_k);
            fdd_timer().stop("subdomain.inner_products");

            alpha_k = gamma_k / theta_k;

            fdd_timer().start("subdomain.vector_operations");
            solution_and_residual_update(u_k, r_kp1, r_k, p_k, q_k, alpha_k);
            fdd_timer().stop("subdomain.vector_operations");

            fdd_timer().start("subdomain.residual_norm");
            residual_norm(r_norm, r_kp1);
            fdd_timer().stop("subdomain.residual_norm");

            iter++;
            residual_history.push_back(r_norm);
            if (print_history) pstdout("- Iter %3d: | residual_norm = %24.16g | relative_residual_norm = %24.16g | \n", iter, r_norm, r_norm / r_0_norm);

            if (use_relative)
            {
                if (r_norm / r_0_norm < tolerance) break;
            }
            else
            {
                if (r_norm < tolerance) break;
            }

            if (iter == max_iterations) break;

            fdd_timer().start("subdomain.preconditioner");
            if (use_preconditioner)
                low_order_preconditioner(z_k, r_kp1);
            else if (use_jacobi)
                jacobi_preconditioner(z_k, r_kp1);
            else
                direct_stiffness_summation(z_k, r_kp1);
            fdd_timer().stop("subdomain.preconditioner");

            fdd_timer().start("subdomain.inner_products");
            search_update_inner_product(theta_k, r_k, r_kp1, z_k);
            fdd_timer().stop("subdomain.inner_products");

            beta_k = theta_k / gamma_k;

            fdd_timer().start("subdomain.vector_operations");
            residual_and_search_update(p_k, r_k, z_k, r_kp1, beta_k);
            fdd_timer().stop("subdomain.vector_operations");
        }

        num_iterations += iter;

        fdd_timer().start("subdomain.vector_operations");
        FDD_CALL(fdd_sub_copy_f64_f64(u_l.as<double>(), u_k.as<double>(), levels[0].num_points, fdd::dev().stream));
        fdd_timer().stop("subdomain.vector_operations");
    }

    // The same flexible GMRES(m) as below (subdomain.tpp:4309-4489), same
    // arithmetic per vector element, restructured around HBM traffic:
    //   - the assembled copy Qt_w V[i] of every basis vector is computed once
    //     and kept (the reference recomputes it inside each of the
    //     (j+1)(j+2)/2 assembled_inner_product calls, subdomain.tpp:4285-4293);
    //   - Qt_w q is computed once per step; the (j+1) dots read it once
    //     (fdd_multi_weighted_inner_product) and come back in one D2H copy;
    //   - the (j+1) Gram-Schmidt updates are one pass over q (fdd_multi_axpy);
    //   - ||q|| is a gather-and-reduce pass with no dof vector in between;
    //   - dssum is the gather-scatter kernel; identity QQt_int is skipped.
    // 4 node passes per step instead of 3 + 2(j+1) + 1 SpMVs.
    bool can_restructure() const
    {
        return not is_composite and subdomain_operator.Qt.unit_values and QQt_int.is_identity and superdomain_operator.num_extended_dofs == 0 and not use_preconditioner and not use_jacobi and num_vectors <= FDD_MULTI_MAX;
    }

    void gather_weighted(fdd::memory &t, fdd::memory &v)
    {
        subdomain_operator.Qt.gather_scatter(nullptr, t.as<double>(), v.as<double>(), norm_weight_is_one ? nullptr : norm_weight.as<double>(), nullptr, 0, subdomain_operator.num_extended_dofs, 1);
    }

    void gather_norm(DType &r_norm, fdd::memory &r)
    {
        subdomain_operator.Qt.gather_weighted_norm2(scalars.as<double>(), reduce_ws.as<double>(), r.as<double>(), norm_weight.as<double>());
        fetch_scalars(&r_norm, 1);
        r_norm = std::sqrt(r_norm);
    }

    void gmres_restructured(fdd::memory &u_l, fdd::memory &f_l, bool print_history, bool use_relative)
    {
        const int nd = subdomain_operator.num_extended_dofs;
        if ((int)Z.size() != num_vectors) allocate_krylov();
        krylov64.ensure(num_vectors, std::max(nd, 1), false);
        std::vector<fdd::memory> &VA = krylov64.VA;
        fdd::memory &qa = krylov64.qa;
        begin_inner_solve();

        tree_operator(f, f_l);
        initialize_arrays(u_k, r_k, f);

        auto norm_of = [&](fdd::memory &v) {
            DType norm;
            gather_norm(norm, v);
            return norm;
        };
        std::vector<double> coeffs(num_vectors + 1);
        std::vector<const double *> ptrs(num_vectors + 1);
        fdd::GmresSpace<DType> space;
        space.initial_norm = [&] { return norm_of(r_k); };
        space.restart_norm = [&] {
            stiffness_matrix(r_k, u_k);
            math.vector_vector_addition(r_k, 1.0, f, -1.0, r_k, num_values);
            return norm_of(r_k);
        };
        space.start_cycle = [&](DType gamma_0) {
            math.vector_scaling(V[0], 1.0 / gamma_0, r_k, num_values);
            gather_weighted(VA[0], V[0]);
        };
        space.arnoldi_step = [&](int j, std::vector<std::vector<DType>> &H) {
            direct_stiffness_summation(Z[j], V[j]);
            stiffness_matrix(q_k, Z[j]);

            // H[0..j][j] = <q, V[i]> for all i from the same q (classical Gram-Schmidt)
            gather_weighted(qa, q_k);
            for (int i = 0; i < j + 1; i++) ptrs[i] = VA[i].template as<double>();
            {
                fdd::ProfileScope prof("reduce_vec2_kernel<MultiDotW>", 8.0 * nd * (j + 3));
                FDD_CALL(fdd_multi_weighted_inner_product(scalars.as<double>(), reduce_ws.as<double>(), qa.as<double>(), ptrs.data(), j + 1, norm_weight.as<double>(), nd, fdd::dev().stream));
            }
            fetch_scalars(coeffs.data(), j + 1);
            for (int i = 0; i < j + 1; i++)
            {
                H[i][j] = coeffs[i];
                coeffs[i] = -H[i][j];
                ptrs[i] = V[i].template as<double>();
            }
            {
                fdd::ProfileScope prof("ew_vec2_kernel<MultiAxpy>", 8.0 * num_values * (j + 3));
                FDD_CALL(fdd_multi_axpy(q_k.as<double>(), coeffs.data(), ptrs.data(), j + 1, num_values, fdd::dev().stream));
            }
            return norm_of(q_k);
        };
        space.next_vector = [&](int j, DType alpha_j) {
            math.vector_scaling(V[j + 1], 1.0 / alpha_j, q_k, num_values);
            gather_weighted(VA[j + 1], V[j + 1]);
        };
        space.add_update = [&](int j, const std::vector<DType> &c) {
            for (int i = 0; i < j + 1; i++) ptrs[i] = Z[i].template as<double>();
            fdd::ProfileScope prof("ew_vec2_kernel<MultiAxpy>", 8.0 * num_values * (j + 3));
            FDD_CALL(fdd_multi_axpy(u_k.as<double>(), c.data(), ptrs.data(), j + 1, num_values, fdd::dev().stream));
        };
        num_iterations += fdd::gmres_solve(gmres_scalars, num_vectors, inner_gmres_control(use_relative), space, residual_history, print_inner_step(print_history));

        FDD_CALL(fdd_sub_copy_f64_f64(u_l.as<double>(), u_k.as<double>(), levels[0].num_points, fdd::dev().stream));
    }

    // ------------------------------------------------------------------
    // The same flexible GMRES(m) once more, with every Krylov vector held
    // ASSEMBLED (one value per dof instead of one per element-local point).
    // The reference's point-space iteration only ever looks at its vectors
    // through Qt: the inner products are <Qt u, Qt v> (subdomain.tpp:4277-4307),
    // the operator is A Q Qt (dssum, then the element stiffness), so with
    // v~ = Qt v it IS GMRES on Qt A Q in the dof space, and its result is
    // u = Q u~.  Per step: the element stiffness reads Q z~ through the
    // point -> dof index array (no dssum pass, no point-space copy), one gather
    // Qt back to the dofs, then dots / update / norm / scaling on dof vectors
    // (0.68x the points at N = 7) with the Gram-Schmidt coefficients and the
    // norm staying on the device: one host synchronisation per step.
    // Same recurrences and Givens rotations as subdomain.tpp:4309-4489; the
    // iterates agree with the point-space form to rounding (Qt is applied
    // before instead of after the linear combinations).
    // ------------------------------------------------------------------
    bool can_assemble() const
    {
        if (is_composite) return false;
        if (not(subdomain_operator.Qt.unit_values and QQt_int.is_identity and superdomain_operator.num_extended_dofs == 0 and num_vectors <= FDD_MULTI_MAX and dim == 3)) return false;
        for (auto &ll : subdomain_operator.level_lists)
            if (ll.poly_degree > 15) return false;
        return true;
    }

    // ---- affine elements (an option of this build, see Domain::set_affine_geometry) ----
    // Every level list of the region (own elements, rings at their reduced degrees) is checked on its own: a list whose
    // factor arrays all have the form c_f(e) (w_i w_j) w_k to rounding runs on the kernel that does not stream them.
    // Returns the number of lists switched over.
    const std::vector<fdd::LevelList> &operator_lists() const { return subdomain_operator.level_lists; }
    // how many of them the gather form of the precision in use runs on a kernel of the given kind (fddh_problem_*_info); a float
    // inner solve has no matrix-core kernel
    int count_lists(bool (fdd::StiffnessChoice::*is)() const) const
    {
        int count = 0;
        for (auto &ll : subdomain_operator.level_lists)
            if ((fdd::choose_stiffness(ll, stiffness, precision == 32, fdd::StiffnessForm::gather).*is)()) count++;
        return count;
    }
    int set_affine_geometry(bool on)
    {
        int count = 0;
        for (auto &ll : subdomain_operator.level_lists)
        {
            ll.affine_requested = on;
            ll.affine = on and fdd::detect_affine(ll);
            fdd::affine_float_copies(ll); // of a checked list, for the single-precision inner solve
            if (ll.affine) count++;
        }
        return count;
    }

    void gmres_assembled(fdd::memory &u_l, fdd::memory &f_l, bool print_history, bool use_relative)
    {
        const int nd = std::max(dof_alloc_size(), 1);
        fdd::memory &ua = krylov64.ua, &fa = krylov64.fa;
        if (not ua.ptr()) ua = fdd::dev().malloc<DType>(nd);
        if (not fa.ptr()) fa = fdd::dev().malloc<DType>(nd);
        if (is_composite)
        {
            // the composite in dof space (setup_composite_dofs): same iteration, its vectors over the unique dofs
            gmres_composite_dofs(ua, f_l, print_history, use_relative);
            composite_solution_points(u_l, ua);
            return;
        }
        // f~ = Qt T f (the degree tree runs as in the reference; its level-0 part is the right-hand side)
        if (build_tree)
        {
            tree_operator(f, f_l);
            gather_weighted(fa, f);
        }
        else
            gather_weighted(fa, f_l);

        gmres_dofs(ua, fa, print_history, use_relative);

        // u = Q u~ on the level-0 points (points without a dof get the 0.0 the SpMV writes)
        fdd::memory u_sub_l = u_l.slice(0, subdomain_operator.num_points);
        subdomain_operator.Q.multiply(u_sub_l, ua);
    }

    // The same solve with the scalar bookkeeping (Hessenberg column, Givens rotations,
    // residual recurrence, stopping tests, back-substitution) in one-thread kernels
    // (fdd_gmres_*_dev): a whole restart cycle is enqueued back to back and the host
    // synchronises ONCE per cycle, to read the history and the stopping column.  A stop
    // inside a cycle is recorded, not acted on: the remaining steps run on vectors
    // nobody uses and the update takes the columns the reference would have taken.
    void gmres_dofs_device(fdd::memory &ua, fdd::memory &fa, bool print_history, bool use_relative, const fdd::InnerSolveHints &hints = {})
    {
        if (inner_solver == 1) return chebyshev_dofs(ua, fa);
        if (precision == 32)
            gmres_dofs_device_t(krylov32, ua, fa, print_history, use_relative, hints);
        else
            gmres_dofs_device_t(krylov64, ua, fa, print_history, use_relative, hints);
    }

    // Real = float is the reference's PTYPE = Float: the same recurrences and the same device bookkeeping on float vectors
    // (prepare_single_precision), with the casts of subdomain.okl:268-282 at the two ends; ua_io / fa_io are double either way.
    template <typename Real>
    void gmres_dofs_device_t(DofKrylov<Real> &K, fdd::memory &ua_io, fdd::memory &fa_io, bool print_history, bool use_relative, const fdd::InnerSolveHints &hints = {})
    {
        constexpr bool f32 = std::is_same<Real, float>::value;
        namespace ops = fdd::ops;
        const int nd = dof_space_size();         // the unique dofs the iteration runs on
        const int na = std::max(dof_alloc_size(), 1); // composite: room for the copies / hanging values behind them
        const int m = num_vectors;
        void *stream = fdd::dev().stream;
        if constexpr (f32) prepare_single_precision();
        const bool jacobi = use_jacobi and not use_preconditioner;
        const bool pre = use_preconditioner or jacobi; // the preconditioned basis Z is kept
        if (jacobi) ensure_jacobi();
        K.ensure(m, na, pre);
        if constexpr (f32)
        {
            if (not K.ua.ptr()) K.ua = fdd::dev().malloc<float>(na);
            if (not K.fa.ptr()) K.fa = fdd::dev().malloc<float>(na);
            FDD_CALL(fdd_sub_copy_f32_f64(K.fa.template as<float>(), fa_io.as<double>(), nd, stream)); // copy_from_domain_data, subdomain.okl:268-274
        }
        Real *ua = (f32 ? K.ua : ua_io).template as<Real>(), *fa = (f32 ? K.fa : fa_io).template as<Real>(), *qa = K.qa.template as<Real>();
        if (not gmres_state.ptr())
        {
            // cleared once: the counters of fdd_gmres_step_last_dev live as long as the state (every member is a double)
            gmres_state = fdd::dev().malloc<char>(fdd_gmres_state_bytes());
            FDD_CALL(fdd_set_to_value(gmres_state.as<double>(), 0.0, (int)(fdd_gmres_state_bytes() / sizeof(double)), 0, fdd::dev().stream));
        }
        begin_inner_solve();
        double *sc = scalars.as<double>();
        double *ws = reduce_ws.as<double>();
        // NULL: unit weights, not read (the composite iterates on its unique dofs: all weights 1; the float reductions take none)
        const double *nw = (f32 or norm_weight_is_one or is_composite) ? nullptr : norm_weight.as<double>();
        void *st = gmres_state.ptr();
        const double *y_dev = nullptr, *inv_dev = nullptr;
        FDD_CALL(fdd_gmres_coefficients(st, &y_dev));
        FDD_CALL(fdd_gmres_scales(st, &inv_dev));

        // the float solve runs the float V-cycle and gives and takes float vectors (f32_io); the double one gives and
        // takes double vectors whatever the cycle's own precision
        if (use_preconditioner)
        {
            if constexpr (f32)
            {
                amg_checked();
                if (amg_hierarchy.precision != 32 and not amg_hierarchy.set_precision(32))
                {
                    fprintf(stderr, "ERROR: the single-precision preconditioner needs a Chebyshev order of at least 2\n");
                    exit(EXIT_FAILURE);
                }
                amg_hierarchy.set_f32_io(true);
            }
            else if (amg_hierarchy.f32_io)
                amg_hierarchy.set_f32_io(false);
        }

        // The basis is kept UNNORMALISED: W_j = r (j = 0) or the orthogonalised q (j > 0), with
        // inv[j] = 1/gamma_0 or 1/||q|| in the device state.  Every reader forms inv[j] * W_j[d] on load
        // -- the value vector_scaling would have stored (subdomain.tpp:4358, 4457), bit for bit -- so the
        // normalisation pass per step disappears.
        // u~ starts at 0 (subdomain.tpp:4270-4275); the first update writes it without reading it
        int iter = 0;
        bool first_cycle = true;
        const bool lazy = hints.lazy_history and max_iterations <= m and fdd::globals().pstdout_file == nullptr;
        std::vector<Real *> W(m + 1), ptrs(m + 1);
        std::vector<double> hist(FDD_MULTI_MAX + 1);

        while (iter < max_iterations)
        {
            if (first_cycle)
                W[0] = fa; // read only
            else
            {
                // r~ = f~ - Qt A Q u~
                operator_dofs(qa, ua);
                W[0] = K.VA[0].template as<Real>();
                ops::vector_vector_addition(W[0], 1, fa, -1, qa, nd, stream);
            }
            if (not f32 and first_cycle and hints.known_rhs_norm2 and nw == nullptr)
                FDD_CALL(fdd_gmres_begin_dev(st, hints.known_rhs_norm2, 1, stream)); // the caller has just formed |f~|^2 with this very call (Domain::node_norm_enqueue)
            else
            {
                ops::multi_dot(sc, ws, W[0], W.data(), nullptr, 1, nw, nd, stream);
                FDD_CALL(fdd_gmres_begin_dev(st, sc, first_cycle ? 1 : 0, stream));
            }

            for (int j = 0; j < m; j++)
            {
                Real *za = pre ? K.ZA[j].template as<Real>() : W[j];
                if (use_preconditioner)
                {
                    // z~_j = V(inv_j W_j): the V-cycle wants the normalised vector in its own buffer anyway
                    Real *rhs;
                    if constexpr (f32)
                        rhs = amg_hierarchy.rhs32().template as<float>();
                    else
                        rhs = amg_checked().f.template as<double>();
                    ops::scaling_dev(rhs, inv_dev + j, W[j], nd, stream);
                    amg_hierarchy.vcycle_into(K.ZA[j]); // the correction lands in the preconditioned basis vector itself
                }
                else if (jacobi) // z~_j = D^-1 (inv_j W_j)
                    ops::diagonal_scaling_dev(za, (f32 ? jacobi_dinv_f32 : jacobi_dinv).template as<Real>(), inv_dev + j, W[j], nd, stream);
                operator_dofs(qa, za, pre ? nullptr : inv_dev + j);

                double *slot = sc + (j & 1) * FDD_GMRES_SLOT;
                W[j + 1] = K.VA[j + 1].template as<Real>();
                if constexpr (not f32)
                    if (norm_from_projections_at(j))
                    {
                        // the cycle's last vector is never read and its norm is <q, q> - sum h^2 up to rounding: the dots carry
                        // <q, q> along (slot[j + 1]), the exact pass is gated on those numbers on the device (it writes
                        // slot[j + 2] where it runs), and the step asks the same function which of the two to take.  With the
                        // vector stored the pass runs ungated for the vector; the norm is chosen the same way.
                        ops::multi_dot_self(slot, ws, qa, W.data(), inv_dev, j + 1, nw, nd, stream);
                        if (skip_last_basis_store)
                            ops::multi_axpy_norm2_gated(slot + (j + 2), ws, nullptr, qa, slot, -1.0, W.data(), inv_dev, j + 1, nw, nd, slot, stream);
                        else
                            ops::multi_axpy_norm2(slot + (j + 2), ws, W[j + 1], qa, slot, -1.0, W.data(), inv_dev, j + 1, nw, nd, stream);
                        FDD_CALL(fdd_gmres_step_last_dev(st, slot, j, iter, max_iterations, tolerance, use_relative ? 1 : 0, stream));
                        continue;
                    }
                ops::multi_dot(slot, ws, qa, W.data(), inv_dev, j + 1, nw, nd, stream);
                // the cycle's last basis vector is never read: only its norm is formed
                ops::multi_axpy_norm2(slot + (j + 1), ws, (j + 1 < m or not skip_last_basis_store) ? W[j + 1] : nullptr, qa, slot, -1.0, W.data(), inv_dev, j + 1, nw, nd, stream);
                FDD_CALL(fdd_gmres_step_dev(st, slot, j, iter, max_iterations, tolerance, use_relative ? 1 : 0, stream));
            }
            FDD_CALL(fdd_gmres_finish_dev(st, m, stream));

            for (int i = 0; i < m; i++) ptrs[i] = pre ? K.ZA[i].template as<Real>() : W[i];
            const double *scales = pre ? nullptr : inv_dev;
            if (lazy)
            {
                // single cycle, nobody is waiting for the history: the update takes its column count from the
                // device state and the host does not synchronise at all (finish_history() reads the state later)
                const double *last_dev = nullptr;
                FDD_CALL(fdd_gmres_last_column(st, &last_dev));
                bool deferred = false;
                if constexpr (not f32)
                    if (fdd::PendingUpdate *pu = hints.defer_into)
                    {
                        // the caller launches it, inside the pass that reads u~ first (Domain::fcg_nodes_step_direction)
                        pu->active = deferred = true;
                        pu->q = ua, pu->q_is_zero = 1, pu->n = nd;
                        pu->coeffs_dev = y_dev, pu->scales_dev = scales, pu->last_dev = last_dev;
                        pu->v.assign(ptrs.begin(), ptrs.begin() + m);
                    }
                if (not deferred) ops::lincomb_limited(ua, 1, y_dev, ptrs.data(), scales, last_dev, m, nd, stream);
                history_pending = true;
                iter = std::min(m, max_iterations); // the steps enqueued; an early stop is only known to the device
                break;
            }

            // the one synchronisation of the cycle
            int nh = 0, j_last = -1, steps = 0, converged = 0;
            FDD_CALL(fdd_gmres_fetch(st, nullptr, hist.data(), &nh, &j_last, &steps, &converged, stream));
            if (first_cycle)
            {
                residual_history.push_back(hist[0]);
                if (print_history) pstdout("- Iter %3d: | residual_norm = %24.16g | relative_residual_norm = %24.16g | \n", 0, hist[0], 1.0);
            }
            for (int k = 1; k < nh; k++)
            {
                residual_history.push_back(hist[k]);
                if (print_history) pstdout("- Iter %3d: | residual_norm = %24.16g | relative_residual_norm = %24.16g | \n", iter + k, hist[k], hist[k] / residual_history[0]);
            }
            iter += steps;

            if (j_last >= 0)
                ops::lincomb(ua, first_cycle ? 1 : 0, y_dev, ptrs.data(), scales, j_last + 1, nd, stream);
            else if (first_cycle)
                ops::set_to_zero(ua, nd, stream);
            first_cycle = false;
            if (converged) break;
        }
        if constexpr (f32) FDD_CALL(fdd_sub_copy_f64_f32(ua_io.as<double>(), ua, nd, stream)); // copy_to_domain_data, subdomain.okl:276-282
        num_iterations += iter;
    }

    // ------------------------------------------------------------------
    // CHEBYSHEV-JACOBI inner solve -- a LABELLED OPTION of this build (inner_solver = 1), not in the reference, which runs
    // the Chebyshev recurrence on the CSR levels of the V-cycle only (subdomain.tpp:19-83).  u~ = p_m(D^-1 A) D^-1 f~ with
    // p_m the Chebyshev polynomial of the interval [lower, upper] * lambda, D the exact diagonal of ensure_jacobi and
    // lambda a Rayleigh quotient of D^-1/2 A D^-1/2 (chebyshev_lambda).  From x = 0, with theta = (a + b)/2,
    // delta = (b - a)/2, sigma = theta/delta, rho_0 = 1/sigma:
    //   k = 0       : d = w .* f, w = 1 / (theta diag) formed once on the host     x = d
    //                 (one rounding fewer than (1/theta) (dinv .* f): the order-1 solve is within 1 ulp of f / (theta diag))
    //   k = 1..m-1  : r = r_prev - A d (r_prev = f at k = 1: f is never written)
    //                 rho_k = 1/(2 sigma - rho_{k-1});  d = rho_k rho_{k-1} d + (2 rho_k/delta) D^-1 r;   x = x + d
    // m diagonal scalings, m - 1 operator applications, no inner product, no host synchronisation: M^-1 is a fixed,
    // symmetric, linear operator.  The coefficients are formed here in double and passed by value.  One pass per step
    // (fdd_cheby_step), in a conforming region as the epilogue of the gather Qt that ends the operator application
    // (fdd_csr_plan_gather_cheby), or composed from vector_vector_addition / diagonal_scaling where the kernel library
    // has neither: the same bits in all three.  The history stays empty; the caller's InnerSolveHints are not looked
    // at (x is written in place, no update is left pending).
    // ------------------------------------------------------------------
    // why this problem cannot run it, or nullptr
    const char *chebyshev_refusal() const
    {
        if (use_preconditioner) return "inner_solver = 1 (Chebyshev-Jacobi) with sub_use_preconditioner = 1: the Chebyshev iteration around the V-cycle is not part of this build (use sub_use_preconditioner 0 or 2)";
        if (not dof_space_available()) return "inner_solver = 1 (Chebyshev-Jacobi) needs the dof-space inner solve: a 3-D region with assembled_inner_solve = 1";
        return nullptr;
    }

    // lambda: the Rayleigh quotient after cheby.power_iterations steps of the power iteration on S A S, S = 1/sqrt(diag)
    // (device_power_iteration, with operator_dofs as the operator).  The region is the rank's own operator: no
    // communication.  Kept until the operator changes (operator_changed) or the iteration count does.
    double chebyshev_lambda()
    {
        if (cheby.lambda > 0.0) return cheby.lambda;
        ensure_jacobi();
        const int nd = dof_space_size(), na = std::max(dof_alloc_size(), 1);
        if (nd <= 0 or cheby.power_iterations <= 0) return cheby.lambda = 1.0;
        std::vector<double> s_hst(nd);
        for (int i = 0; i < nd; i++) s_hst[i] = 1.0 / std::sqrt(jacobi_diag_hst[i]);
        fdd::memory S = fdd::dev().malloc<double>(nd);
        S.copyFrom(s_hst.data(), (size_t)nd * sizeof(double));
        const double lambda = device_power_iteration(nd, na, S, cheby.power_iterations, [this](fdd::memory &w, fdd::memory &t) { operator_dofs(w.as<double>(), t.as<double>()); });
        if (not(lambda > 0.0) or not std::isfinite(lambda)) throw std::runtime_error("Chebyshev-Jacobi inner solve: the power iteration gave no positive eigenvalue estimate");
        return cheby.lambda = lambda;
    }

    void chebyshev_dofs(fdd::memory &ua, fdd::memory &fa)
    {
        if (const char *why = chebyshev_refusal()) throw std::runtime_error(why);
        if (precision == 32)
            chebyshev_dofs_t(cheby32, ua, fa);
        else
            chebyshev_dofs_t(cheby64, ua, fa);
    }

    // ua_io / fa_io are double either way (Real = float: the casts of subdomain.okl:268-282 at the two ends); fa_io is read only
    template <typename Real>
    void chebyshev_dofs_t(ChebyVectors<Real> &C, fdd::memory &ua_io, fdd::memory &fa_io)
    {
        constexpr bool f32 = std::is_same<Real, float>::value;
        namespace ops = fdd::ops;
        const int nd = dof_space_size(), na = std::max(dof_alloc_size(), 1), m = cheby.order;
        void *stream = fdd::dev().stream;
        const double lambda = chebyshev_lambda(); // makes the diagonal too
        if constexpr (f32) prepare_single_precision();
        if (C.na != na)
        {
            C.w = fdd::memory(); // made again below, at the new size
            for (fdd::memory *v : {&C.d, &C.r, &C.q, &C.t}) *v = fdd::dev().malloc<Real>(na); // d is an operator input: in a composite the copies and hanging values sit behind its dofs
            if (f32) C.x = fdd::dev().malloc<Real>(na), C.f = fdd::dev().malloc<Real>(na);
            ops::set_to_zero(C.d.template as<Real>(), na, stream);
            C.na = na;
        }
        if constexpr (f32) FDD_CALL(fdd_sub_copy_f32_f64(C.f.template as<float>(), fa_io.as<double>(), nd, stream));
        Real *x = (f32 ? C.x : ua_io).template as<Real>(), *d = C.d.template as<Real>(), *r = C.r.template as<Real>(), *q = C.q.template as<Real>(), *t = C.t.template as<Real>();
        const Real *f = (f32 ? C.f : fa_io).template as<Real>();
        const Real *dinv = (f32 ? jacobi_dinv_f32 : jacobi_dinv).template as<Real>();
        begin_inner_solve();

        const bool kernels = cheby.use_kernels and fdd::missing_chebyshev_entry(false) == nullptr;
        // the float gather takes no norm weight; the double one may: then the separate pass stays.  So it does with a Helmholtz
        // shift: the gather's epilogue would take q before the term is added (operator_dofs adds it)
        const bool fused = kernels and cheby.fused and not is_composite and not shift_active() and (f32 or norm_weight_is_one) and subdomain_operator.Qt.num_rows == nd and subdomain_operator.Qt.gather_cheby_applies();
        const double a = cheby.lower * lambda, b = cheby.upper * lambda, theta = 0.5 * (a + b), delta = 0.5 * (b - a), sigma = theta / delta;
        double rho = 1.0 / sigma;

        // k = 0, with the scaling 1 / (theta diag) of this interval and this diagonal and the factor 1
        if (not C.w.ptr() or C.w_theta != theta or C.w_generation != operator_generation)
        {
            std::vector<Real> w_hst(std::max(nd, 1), Real(1));
            for (int i = 0; i < nd; i++) w_hst[i] = (Real)(1.0 / (theta * jacobi_diag_hst[i]));
            if (not C.w.ptr()) C.w = fdd::dev().malloc<Real>(w_hst.size());
            C.w.copyFrom(w_hst.data(), w_hst.size() * sizeof(Real));
            C.w_theta = theta;
            C.w_generation = operator_generation;
        }
        const Real *w = C.w.template as<Real>();
        if (kernels)
            ops::cheby_step(x, d, (Real *)nullptr, f, (const Real *)nullptr, w, 0.0, 1.0, true, m == 1, nd, stream);
        else
        {
            ops::diagonal_scaling_dev(t, w, nullptr, f, nd, stream);
            ops::vector_vector_addition(m == 1 ? x : d, (Real)1, t, (Real)0, t, nd, stream);
            if (m > 1) ops::copy(x, d, nd, stream);
        }
        for (int k = 1; k < m; k++)
        {
            const double rho_k = 1.0 / (2.0 * sigma - rho), c_d = rho_k * rho, c_r = 2.0 * rho_k / delta;
            const Real *r_in = k == 1 ? f : r;
            const bool last = k == m - 1;
            if (fused)
            {
                Real *q_pts = (f32 ? sp.q_pts : q_k).template as<Real>();
                stiffness_from_dofs(q_pts, d);
                subdomain_operator.Qt.gather_cheby(x, d, r, q_pts, r_in, dinv, c_d, c_r, last);
            }
            else
            {
                operator_dofs(q, d);
                if (kernels)
                    ops::cheby_step(x, d, r, r_in, q, dinv, c_d, c_r, false, last, nd, stream);
                else
                {
                    Real *rr = last ? t : r; // the last step stores neither r nor d
                    ops::vector_vector_addition(rr, (Real)1, r_in, (Real)-1, q, nd, stream);
                    ops::diagonal_scaling_dev(t, dinv, nullptr, rr, nd, stream);
                    Real *dn = last ? t : d;
                    ops::vector_vector_addition(dn, (Real)c_d, d, (Real)c_r, t, nd, stream);
                    ops::vector_vector_addition(x, (Real)1, x, (Real)1, dn, nd, stream);
                }
            }
            rho = rho_k;
        }
        if constexpr (f32) FDD_CALL(fdd_sub_copy_f64_f32(ua_io.as<double>(), x, nd, stream));
        num_iterations += m;
    }

    // test hook: the configured inner solve on host dof vectors of dof_count() values
    void host_solve_dofs(double *ua_hst, const double *fa_hst)
    {
        const int nd = dof_space_size(), na = std::max(dof_alloc_size(), 1);
        fdd::memory fa = fdd::dev().malloc<DType>(na), ua = fdd::dev().malloc<DType>(na);
        FDD_CALL(fdd_set_to_value(fa.as<double>(), 0.0, na, 0, fdd::dev().stream));
        FDD_CALL(fdd_set_to_value(ua.as<double>(), 0.0, na, 0, fdd::dev().stream));
        fa.copyFrom(fa_hst, (size_t)nd * sizeof(DType));
        if (is_composite)
            gmres_dofs_device(ua, fa, false, false);
        else
            gmres_dofs(ua, fa, false, false);
        finish_history();
        ua.copyTo(ua_hst, (size_t)nd * sizeof(DType));
    }

    // the solve itself, dof vectors in and out (callers that already hold assembled data skip Qt / Q)
    void gmres_dofs(fdd::memory &ua, fdd::memory &fa, bool print_history = true, bool use_relative = false, const fdd::InnerSolveHints &hints = {})
    {
        if (inner_solver == 1) return chebyshev_dofs(ua, fa);
        if (device_bookkeeping and num_vectors <= FDD_MULTI_MAX)
        {
            gmres_dofs_device(ua, fa, print_history, use_relative, hints);
            return;
        }
        const int nd = subdomain_operator.num_extended_dofs;
        const int m = num_vectors;
        void *stream = fdd::dev().stream;
        const bool jacobi = use_jacobi and not use_preconditioner;
        const bool pre = use_preconditioner or jacobi;
        if (jacobi) ensure_jacobi();
        krylov64.ensure(m, std::max(nd, 1), pre);
        std::vector<fdd::memory> &VA = krylov64.VA, &ZA = krylov64.ZA;
        fdd::memory &qa = krylov64.qa;
        begin_inner_solve();
        double *sc = scalars.as<double>();
        double *ws = reduce_ws.as<double>();
        const double *nw = norm_weight_is_one ? nullptr : norm_weight.as<double>(); // NULL: unit weights, not read

        auto dot_dofs = [&](double *out_dev, fdd::memory &a, const double *const *b, int count) {
            fdd::ProfileScope prof("reduce_vec2_kernel<MultiDotW>", 8.0 * nd * (count + 1 + (nw ? 1 : 0)));
            FDD_CALL(fdd_multi_weighted_inner_product(out_dev, ws, a.as<double>(), b, count, nw, nd, stream));
        };

        FDD_CALL(fdd_set_to_value(ua.as<double>(), 0.0, nd, 0, stream));

        auto norm_of = [&](fdd::memory &v) {
            const double *self[1] = {v.as<double>()};
            DType norm;
            dot_dofs(sc, v, self, 1);
            fetch_scalars(&norm, 1);
            return std::sqrt(norm);
        };
        std::vector<double> coeffs(m + 3);
        std::vector<const double *> ptrs(m + 1);
        fdd::memory *ra = &fa; // assembled residual of the current cycle
        fdd::GmresSpace<DType> space;
        space.initial_norm = [&] { return norm_of(fa); };
        // r~ = f~ - Qt A Q u~
        space.restart_norm = [&] {
            stiffness_from_dofs(q_k.as<double>(), ua.as<double>());
            gather_weighted(qa, q_k);
            FDD_CALL(fdd_vector_vector_addition(qa.as<double>(), 1.0, fa.as<double>(), -1.0, qa.as<double>(), nd, stream));
            ra = &qa;
            return norm_of(qa);
        };
        space.start_cycle = [&](DType gamma_0) { FDD_CALL(fdd_vector_scaling(VA[0].template as<double>(), 1.0 / gamma_0, ra->template as<double>(), nd, stream)); };
        space.arnoldi_step = [&](int j, std::vector<std::vector<DType>> &H) {
            // z~_j = M^-1 v~_j: the identity on assembled data (dssum), or the AMG V-cycle over the dofs
            fdd::memory *za = &VA[j];
            if (use_preconditioner)
            {
                amg::Level &fine = amg_checked();
                fine.f.copyFrom(VA[j], (size_t)nd * sizeof(DType));
                amg_hierarchy.vcycle();
                ZA[j].copyFrom(fine.u, (size_t)nd * sizeof(DType));
                za = &ZA[j];
            }
            else if (jacobi)
            {
                FDD_CALL(fdd_vector_diagonal_scaling_dev(ZA[j].template as<double>(), jacobi_dinv.as<double>(), nullptr, VA[j].template as<double>(), nd, stream));
                za = &ZA[j];
            }

            stiffness_from_dofs(q_k.as<double>(), za->template as<double>());
            gather_weighted(qa, q_k);

            // H[0..j][j] = <q~, v~_i>, q~ -= sum H v~_i, ||q~||^2: coefficients never leave the device in between
            for (int i = 0; i < j + 1; i++) ptrs[i] = VA[i].template as<double>();
            if (norm_from_projections_at(j))
            {
                // the decision of gmres_dofs_device_t at this step, on the fetched numbers: <q~, q~> rides behind the dots, and
                // the exact pass with its second fetch runs only where the function says so (the same bits either way)
                {
                    fdd::ProfileScope prof("reduce_vec2_kernel<MultiDotW>", 8.0 * nd * (j + 2 + (nw ? 1 : 0)));
                    FDD_CALL(fdd_multi_weighted_inner_product_self(sc, ws, qa.as<double>(), ptrs.data(), nullptr, j + 1, nw, nd, stream));
                }
                fetch_scalars(coeffs.data(), j + 2);
                for (int i = 0; i < j + 1; i++) H[i][j] = coeffs[i];
                double est = 0.0;
                const bool usable = fdd_norm2_from_projections(coeffs[j + 1], coeffs.data(), j + 1, &est) != 0;
                const double ratio = est / coeffs[j + 1];
                if (ratio == ratio and (host_norm_estimated + host_norm_exact == 0 or ratio < host_min_ratio)) host_min_ratio = ratio;
                (usable ? host_norm_estimated : host_norm_exact)++;
                if (usable) return std::sqrt(est);
                {
                    fdd::ProfileScope prof("reduce_vec2_kernel<MultiAxpyNorm>", 8.0 * nd * (j + 3 + (nw ? 1 : 0)));
                    FDD_CALL(fdd_multi_axpy_norm2_dev(sc + (j + 2), ws, qa.as<double>(), sc, -1.0, ptrs.data(), j + 1, nw, nd, stream));
                }
                fetch_scalars(coeffs.data(), j + 3);
                return std::sqrt(coeffs[j + 2]);
            }
            dot_dofs(sc, qa, ptrs.data(), j + 1);
            {
                fdd::ProfileScope prof("reduce_vec2_kernel<MultiAxpyNorm>", 8.0 * nd * (j + 3 + (nw ? 1 : 0)));
                FDD_CALL(fdd_multi_axpy_norm2_dev(sc + (j + 1), ws, qa.as<double>(), sc, -1.0, ptrs.data(), j + 1, nw, nd, stream));
            }
            // v~_{j+1} = q~ / ||q~||, launched before the host looks at the numbers (unused if this was the last step)
            FDD_CALL(fdd_vector_scaling_rsqrt_dev(VA[j + 1].template as<double>(), sc + (j + 1), qa.as<double>(), nd, stream));

            fetch_scalars(coeffs.data(), j + 2); // the one synchronisation of the step
            for (int i = 0; i < j + 1; i++) H[i][j] = coeffs[i];
            return std::sqrt(coeffs[j + 1]);
        };
        // already enqueued
        space.next_vector = [](int, DType) {};
        space.add_update = [&](int j, const std::vector<DType> &c) {
            for (int i = 0; i < j + 1; i++) ptrs[i] = pre ? ZA[i].template as<double>() : VA[i].template as<double>();
            fdd::ProfileScope prof("ew_vec2_kernel<MultiAxpy>", 8.0 * nd * (j + 3));
            FDD_CALL(fdd_multi_axpy(ua.as<double>(), c.data(), ptrs.data(), j + 1, nd, stream));
        };
        num_iterations += fdd::gmres_solve(gmres_scalars, m, inner_gmres_control(use_relative), space, residual_history, print_inner_step(print_history));
    }

    // subdomain.tpp:4309-4489
    void generalized_minimum_residual(fdd::memory &u_l, fdd::memory &f_l, bool print_history = true, bool use_relative = false)
    {
        if (inner_solver == 1)
            if (const char *why = chebyshev_refusal()) throw std::runtime_error(why);
        if ((assembled_inner and can_assemble()) or composite_dof_space())
        {
            gmres_assembled(u_l, f_l, print_history, use_relative);
            return;
        }
        if (restructured and fused_dssum and can_restructure())
        {
            gmres_restructured(u_l, f_l, print_history, use_relative);
            return;
        }

        if ((int)Z.size() != num_vectors) allocate_krylov();
        begin_inner_solve();

        tree_operator(f, f_l);

        fdd_timer().start("subdomain.vector_operations");
        initialize_arrays(u_k, r_k, f);
        fdd_timer().stop("subdomain.vector_operations");

        auto norm_of = [&](fdd::memory &v) {
            DType norm;
            fdd_timer().start("subdomain.residual_norm");
            residual_norm(norm, v);
            fdd_timer().stop("subdomain.residual_norm");
            return norm;
        };
        fdd::GmresSpace<DType> space;
        space.initial_norm = [&] { return norm_of(r_k); };
        space.restart_norm = [&] {
            fdd_timer().start("subdomain.operator_application");
            stiffness_matrix(r_k, u_k);
            fdd_timer().stop("subdomain.operator_application");

            fdd_timer().start("subdomain.vector_operations");
            math.vector_vector_addition(r_k, 1.0, f, -1.0, r_k, num_values);
            fdd_timer().stop("subdomain.vector_operations");
            return norm_of(r_k);
        };
        space.start_cycle = [&](DType gamma_0) {
            fdd_timer().start("subdomain.vector_operations");
            math.vector_scaling(V[0], 1.0 / gamma_0, r_k, num_values);
            fdd_timer().stop("subdomain.vector_operations");
        };
        space.arnoldi_step = [&](int j, std::vector<std::vector<DType>> &H) {
            if (use_preconditioner)
            {
                low_order_preconditioner(Z[j], V[j]);
            }
            else if (use_jacobi)
            {
                jacobi_preconditioner(Z[j], V[j]);
            }
            else
            {
                fdd_timer().start("subdomain.preconditioner.identity");
                direct_stiffness_summation(Z[j], V[j]);
                fdd_timer().stop("subdomain.preconditioner.identity");
            }

            fdd_timer().start("subdomain.operator_application");
            stiffness_matrix(q_k, Z[j]);
            fdd_timer().stop("subdomain.operator_application");

            for (int i = 0; i < j + 1; i++)
            {
                fdd_timer().start("subdomain.inner_products");
                assembled_inner_product(H[i][j], q_k, V[i]);
                fdd_timer().stop("subdomain.inner_products");
            }

            for (int i = 0; i < j + 1; i++)
            {
                fdd_timer().start("subdomain.vector_operations");
                math.vector_vector_addition(q_k, 1.0, q_k, -H[i][j], V[i], num_values);
                fdd_timer().stop("subdomain.vector_operations");
            }
            return norm_of(q_k);
        };
        space.next_vector = [&](int j, DType alpha_j) {
            fdd_timer().start("subdomain.vector_operations");
            math.vector_scaling(V[j + 1], 1.0 / alpha_j, q_k, num_values);
            fdd_timer().stop("subdomain.vector_operations");
        };
        space.add_update = [&](int j, const std::vector<DType> &c) {
            for (int i = 0; i < j + 1; i++)
            {
                fdd_timer().start("subdomain.vector_operations");
                math.vector_vector_addition(u_k, 1.0, u_k, c[i], Z[i], num_values);
                fdd_timer().stop("subdomain.vector_operations");
            }
        };
        num_iterations += fdd::gmres_solve(gmres_scalars, num_vectors, inner_gmres_control(use_relative), space, residual_history, print_inner_step(print_history));

        fdd_timer().start("subdomain.vector_operations");
        FDD_CALL(fdd_sub_copy_f64_f64(u_l.as<double>(), u_k.as<double>(), levels[0].num_points, fdd::dev().stream));
        fdd_timer().stop("subdomain.vector_operations");
    }

    // test / analysis hooks on the dof-space form of the inner iteration: y = (Qt A_L Q | A_sup) x on host vectors of
    // dof_count() values, and the dof-space right-hand side of an outer point vector
    int dof_count() const { return dof_space_size(); }
    bool dof_space_available() const { return (assembled_inner and can_assemble()) or composite_dof_space(); }
    void host_operator_dofs(double *y, const double *x)
    {
        const int nd = dof_space_size(), na = std::max(dof_alloc_size(), 1);
        fdd::memory xa = fdd::dev().malloc<DType>(na), ya = fdd::dev().malloc<DType>(na);
        FDD_CALL(fdd_set_to_value(xa.as<double>(), 0.0, na, 0, fdd::dev().stream));
        xa.copyFrom(x, (size_t)nd * sizeof(DType));
        operator_dofs(ya.as<double>(), xa.as<double>());
        ya.copyTo(y, (size_t)nd * sizeof(DType));
    }
    void host_rhs_dofs(double *y, fdd::memory &r_pts)
    {
        const int nd = dof_space_size(), na = std::max(dof_alloc_size(), 1);
        fdd::memory ya = fdd::dev().malloc<DType>(na);
        tree_operator(f, r_pts);
        if (is_composite)
            composite_rhs_dofs(ya, f);
        else
            gather_weighted(ya, f);
        ya.copyTo(y, (size_t)nd * sizeof(DType));
    }

    // test hook: tree_operator is private in the reference too
    void apply_tree_operator(fdd::memory &Tu, fdd::memory &u) { tree_operator(Tu, u); }
    void compute_residual_norm(DType &r_norm, fdd::memory &r) { residual_norm(r_norm, r); }
};

#endif
