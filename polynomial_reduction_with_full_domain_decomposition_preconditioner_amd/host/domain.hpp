/*
 * domain.hpp -- Domain<DType>: the outer-solver host class of the reference
 * (domain.hpp:33-145, domain.tpp) with the same public surface --
 * initialize, initial_function, direct_stiffness_summation, stiffness_matrix,
 * flexible_conjugate_gradient<P>, generalized_minimum_residual<P> -- driving
 * the gfx950 kernels through the C-ABI instead of OCCA.
 *
 * What changed underneath (MI355X-first, same arithmetic):
 *   - stiffness_matrix is one fused launch (element_operator.hpp) instead
 *     of two with a global scratch (domain.tpp:605-606);
 *   - every dot product finishes on the device; only the final scalar(s)
 *     cross PCIe (the reference copies one partial per 128 points and sums on
 *     the host, domain.tpp:924-926);
 *   - gslib's gs_add on the boundary prefix (domain.tpp:590-594: D2H, MPI,
 *     H2D) is a device-resident scatter -> all-reduce -> gather on a dense
 *     interface-slot vector (comm.hpp), MPI_Allreduce of scalars is an
 *     all-reduce of a device buffer;
 *   - mesh data can come from memory (MeshData) as well as from the
 *     Nek5000-export files the reference reads (domain.tpp:45-224).
 */
#ifndef FDD_DOMAIN_HPP
#define FDD_DOMAIN_HPP

#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <unordered_map>
#include <vector>

#include "boundary.hpp"
#include "config.hpp"
#include "csr_matrix.hpp"
#include "diffusivity.hpp"
#include "element.hpp"
#include "element_operator.hpp"
#include "field_ops.hpp"
#include "gll.hpp"
#include "gmres.hpp"
#include "math.hpp"
#include "precision_ops.hpp"
#include "projection.hpp"
#include "timer.hpp"

// The "no preconditioner" plugin: Domain's solvers take any type with these
// two methods (domain.tpp:639-642); with use_preconditioner == false neither
// is called.
namespace fdd
{
// An inner solve's final update u~ = sum_k y_k (s_k v_k), described instead of launched: a caller that reads u~ next in a
// pass of its own hands one in (InnerSolveHints::defer_into) and, where `active` comes back set, owes the update
// (Domain::fcg_nodes_step_direction forms it inside the flexible dot's pass).
struct PendingUpdate
{
    bool active = false;
    double *q = nullptr;
    int q_is_zero = 1;
    const double *coeffs_dev = nullptr, *scales_dev = nullptr, *last_dev = nullptr;
    std::vector<const double *> v;
    int n = 0;
};

// What the caller of one inner solve knows about it: arguments of that call, nothing outlives it.
struct InnerSolveHints
{
    const double *known_rhs_norm2 = nullptr; // |f~|^2 over the dofs, already on the device (double-precision device GMRES only)
    bool lazy_history = false;               // a single-cycle solve does not synchronise at all; Subdomain::finish_history() fetches on demand
    PendingUpdate *defer_into = nullptr;     // non-null: the caller can form the final update itself and receives its description here
};
} // namespace fdd

struct NoPreconditioner
{
    void flexible_conjugate_gradient(fdd::memory &, fdd::memory &) {}
    void generalized_minimum_residual(fdd::memory &, fdd::memory &) {}
    // the surface Domain's assembled flexible CG looks at (never taken: can_assemble() is false)
    std::vector<int> point_dof;
    bool assembled_inner = false;
    bool can_assemble() const { return false; }
    int dofs() const { return 0; }
    void gmres_dofs(fdd::memory &, fdd::memory &, bool = true, bool = false, const fdd::InnerSolveHints & = {}) {}
    bool composite() const { return false; }
    bool composite_dof_space() const { return false; }
    int own_dofs() const { return 0; }
    fdd::memory new_dof_vector() { return fdd::dev().malloc<double>(1); }
    fdd::memory tree_points() { return fdd::dev().malloc<double>(1); }
    void comm_probe_coarse() {}
    void comm_probe_ring() {}
    double comm_coarse_bytes() const { return 0.0; }
    double comm_ring_bytes() const { return 0.0; }
    void gmres_composite_dofs(fdd::memory &, fdd::memory &, bool = true, bool = false, const double * = nullptr, const fdd::InnerSolveHints & = {}) {}
    bool unit_norm_weight() const { return false; }
    bool chebyshev() const { return false; }
};

template <typename DType>
class Domain
{
  private:
    // Work arrays (domain.tpp:56-67)
    std::vector<fdd::memory> work_dev;

    // Dirichlet boundary conditions
    fdd::memory dirichlet_mask;

    // Assembly
    CSR_Matrix<DType> Q;
    CSR_Matrix<DType> Qt;
    fdd::memory assembled_weight;

    // Gather scatter (replaces gs_comm / gs_handle, domain.hpp:51-54)
    int num_bdary_nodes = 0;
    int num_interface_slots = 0;
    fdd::memory bdary_slot;       // int[num_bdary_nodes]: slot of each boundary node
    fdd::memory interface_slots;  // double[num_interface_slots]
    // Neighbour form of the same exchange (xGMI is point-to-point, every pair of GPUs has its own link): each peer gets only
    // the nodes the two ranks share, by one grouped send / receive, and every sharer adds a node's copies in ascending rank
    // order.  Buffer (entries of 1 or 2 interleaved vectors): [own prefix | parts to the peers | parts from the peers].
    struct InterfacePeer
    {
        int rank = 0;
        int first = 0; // first entry of this peer's part inside the send region (= inside the receive region)
        int count = 0; // shared nodes
    };
    std::vector<InterfacePeer> iface_peers;
    int iface_shared_entries = 0;          // sum of the peers' counts
    fdd::memory iface_buf;                 // double[2 * (num_bdary_nodes + 2 * iface_shared_entries)]
    fdd::memory iface_gather_index;        // int[num_bdary_nodes + iface_shared_entries]: prefix node of every own / sent entry
    fdd::memory iface_sum_ptr, iface_sum_col; // CSR over the boundary nodes: the entries of iface_buf a node's sum reads, by contributor rank
    std::vector<fdd::ExchangeOp> iface_ops;

    // Reductions
    fdd::memory reduce_ws;
    fdd::memory scalars; // small device buffer for final dot products

    // Solver
    fdd::memory r_k, r_kp1, q_k, z_k, p_k;
    std::vector<fdd::memory> V;
    std::vector<fdd::memory> Z;
    std::vector<fdd::memory> VA; // assembled copies of the outer GMRES basis
    int va_valid = 0;            // VA[0..va_valid) match V of the current cycle
    fdd::GmresScalars<DType> gmres_scalars; // H, rotations, gamma of the outer GMRES: sized per solve, shared by the point-space and the node-space form
    int gmres_point_vectors = 0; // num_vectors the point-space basis V, Z was allocated for

    // The layout of `scalars` in the node-space flexible CG (double slots).  One all-reduce carries a {next gamma, theta}
    // pair together with the norm's two parts, whichever side of them the pair sits on, and the theta of the sequence
    // without early_gamma together with them as well: the adjacencies below.
    static constexpr int SLOT_GAMMA = 0;  // <z, r> from the projection kernel
    static constexpr int SLOT_PQ = 1;     // <p, q>
    static constexpr int SLOT_PAIR_A = 2; // {next gamma, theta}: the pair alternates between A and B (the current gamma must outlive the next)
    static constexpr int SLOT_THETA = 3;  // theta without early_gamma (the second entry of pair A)
    static constexpr int SLOT_NORM = 4;   // the residual norm's boundary-prefix and interior parts
    static constexpr int SLOT_PAIR_B = 6;
    static_assert(SLOT_PAIR_A + 2 == SLOT_NORM and SLOT_NORM + 2 == SLOT_PAIR_B, "a pair and the norm's parts are four contiguous doubles on either side");
    static_assert(SLOT_THETA + 1 == SLOT_NORM and SLOT_THETA == SLOT_PAIR_A + 1, "theta sits right in front of the norm's parts");

    // state of a running flexible CG (fcg_begin / fcg_step / fcg_steps): a fresh one per solve
    struct FcgRun
    {
        fdd::memory u, u_pts; // the solution vector (point space); where fcg_finish puts the solution (node space)
        bool nodes_active = false;
        DType r_0_norm = 0.0, gamma_k = 0.0;
        int iter = 0;
        bool norm_pending = false;                 // device_scalars: the last residual norm is enqueued, not fetched
        const double *pending_rhs_norm2 = nullptr; // what node_norm_enqueue returned for the residual the next precondition_nodes call receives
        bool gamma_on_device = false;
        int gamma_slot = SLOT_GAMMA; // where the current gamma sits in `scalars`
        // u~ += alpha p~ of the iteration whose residual half ran last, not launched yet (solution_in_direction_pass): the
        // direction half carries it in the pass that reads p~ anyway, and whatever reads u~ before that flushes it first
        // (fcg_flush_solution_update).  alpha = *num / *den, both still in `scalars` until the direction half has run
        struct OwedSolutionUpdate
        {
            bool active = false;
            const double *num = nullptr, *den = nullptr;
        };
        OwedSolutionUpdate owed_u;
    };
    FcgRun fcg;

    // the node residual norm in flight (node_norm_enqueue / node_norm_finish): reset where a solve starts
    struct NormInFlight
    {
        int parts = 1;                  // scalars[SLOT_NORM..]: boundary-prefix and interior parts of the last enqueued norm
        bool deferred = false;          // the saved prefix still waits for its exchange
        bool reduce_pending = false;    // the slots still hold this rank's parts only
        const double *source = nullptr; // the vector whose norm is being taken
    };
    NormInFlight norm_state;

    // ---- assembled flexible CG: every vector holds one value per local node ----
    // (see fcg_nodes_* below; built on first use)
    bool nodes_ready = false;
    fdd::memory norm_hist;               // device-side residual history of fcg_steps
    int norm_hist_cap = 0;
    fdd::memory nprefix;                 // the boundary prefix of the norm's vector (exchanged copy)
    fdd::memory point_node_dev;           // int[num_local_points]: Q as an index array
    fdd::memory node_mask;                // Dirichlet mask per node
    fdd::memory node_stitch;              // local multiplicity * assembled weight * mask
    std::vector<DType> node_stitch_hst, node_mask_hst;
    bool norm_on_dof_slice = false;       // one rank, mask = indicator of the dof slice: the masked node norm is the slice's plain norm
    bool stitch_is_one = false;           // every weight of the dof slice is exactly 1.0 (setup_dof_maps)
    fdd::memory node_of_dof, dof_of_node; // renumbering to / from the subdomain's dofs
    int nodes_sub_dofs = -1;
    int dof_shift = -1; // >= 0: subdomain dof d is node d + dof_shift (the numbering makes it so), no renumbering pass
    fdd::memory nu, nr, nr1, nq, nz, np, nt, sub_f, sub_u;
    // node-space outer GMRES (gmres_nodes): f^ = Qt f, the basis and the preconditioned basis as node vectors, with more
    // than one rank the basis once more with the interface prefix summed over the ranks, on a composite the basis on the
    // points as well (the degree tree restricts point data)
    fdd::memory nf;
    std::vector<fdd::memory> VN, ZN, VNA, VP;
    int gmres_nodes_vectors = 0;
    bool composite_rhs_from_nodes = true; // composite preconditioner: own part of its right-hand side = the node residual (no second gather of the own points)
    fdd::memory rp;                 // composite preconditioner: the residual on the element-local points (the degree tree and the ring / superdomain exchange start from it)
    bool composite_precond = false; // the Subdomain is a full-domain-decomposition composite driven in dof space

    Math<DType> math;

    fdd::LevelList list; // the rank's elements as one run of one degree: what the element operator works on (element_operator.hpp)

    // From the all-gathered boundary ids (rank order, counts[r] per rank; every rank holds the same lists, so no further
    // communication): who shares which of this rank's boundary nodes.  Peer parts are ordered by global id on both sides.
    void build_interface_neighbour_plan(const std::vector<long long> &ids_by_rank, const std::vector<int> &counts, const std::vector<long long> &mine)
    {
        const int me = fdd::comm().rank, R = fdd::comm().size, nb = (int)mine.size();
        std::vector<std::pair<long long, int>> holders; // (global id, rank), sorted: the ranks of an id come out ascending
        holders.reserve(ids_by_rank.size());
        size_t at = 0;
        for (int r = 0; r < R; r++)
            for (int k = 0; k < counts[r]; k++, at++) holders.emplace_back(ids_by_rank[at], r);
        std::sort(holders.begin(), holders.end());
        // this rank's boundary nodes by global id
        std::vector<std::pair<long long, int>> own(nb);
        for (int b = 0; b < nb; b++) own[b] = {mine[b], b};
        std::sort(own.begin(), own.end());

        // per peer: the shared nodes in ascending global id (the walk over `own` is in that order)
        std::vector<std::vector<int>> shared(R);      // prefix node
        std::vector<std::vector<int>> sharers(nb);    // ranks holding node b, ascending (this rank included)
        for (int k = 0; k < nb; k++)
        {
            const long long g = own[k].first;
            const int b = own[k].second;
            auto lo = std::lower_bound(holders.begin(), holders.end(), std::make_pair(g, -1));
            for (auto it = lo; it != holders.end() and it->first == g; ++it)
            {
                sharers[b].push_back(it->second);
                if (it->second != me) shared[it->second].push_back(b);
            }
        }
        iface_peers.clear();
        iface_shared_entries = 0;
        std::vector<int> first_of(R, -1);
        for (int r = 0; r < R; r++)
        {
            if (shared[r].empty()) continue;
            InterfacePeer pr;
            pr.rank = r;
            pr.first = iface_shared_entries;
            pr.count = (int)shared[r].size();
            first_of[r] = pr.first;
            iface_shared_entries += pr.count;
            iface_peers.push_back(pr);
        }
        std::vector<int> gidx((size_t)nb + iface_shared_entries);
        for (int b = 0; b < nb; b++) gidx[b] = b;
        std::vector<std::vector<int>> pos(R); // position of node b inside peer r's part
        for (const InterfacePeer &pr : iface_peers)
        {
            pos[pr.rank].assign(nb, -1);
            for (int k = 0; k < pr.count; k++)
            {
                gidx[(size_t)nb + pr.first + k] = shared[pr.rank][k];
                pos[pr.rank][shared[pr.rank][k]] = k;
            }
        }
        std::vector<int> sptr(nb + 1, 0), scol;
        for (int b = 0; b < nb; b++)
        {
            for (int r : sharers[b]) scol.push_back(r == me ? b : nb + iface_shared_entries + first_of[r] + pos[r][b]);
            sptr[b + 1] = (int)scol.size();
        }
        iface_buf = fdd::dev().malloc<double>(2 * ((size_t)nb + 2 * (size_t)iface_shared_entries) + 2);
        iface_gather_index = fdd::dev().malloc<int>(std::max<size_t>(gidx.size(), 1));
        if (not gidx.empty()) iface_gather_index.copyFrom(gidx.data(), gidx.size() * sizeof(int));
        iface_sum_ptr = fdd::dev().malloc<int>(sptr.size());
        iface_sum_ptr.copyFrom(sptr.data(), sptr.size() * sizeof(int));
        iface_sum_col = fdd::dev().malloc<int>(std::max<size_t>(scol.size(), 1));
        if (not scol.empty()) iface_sum_col.copyFrom(scol.data(), scol.size() * sizeof(int));
    }

    // the grouped send / receive of the neighbour form for `nc` interleaved vectors
    void iface_exchange(int nc)
    {
        iface_ops.resize(iface_peers.size());
        double *base = iface_buf.as<double>();
        for (size_t k = 0; k < iface_peers.size(); k++)
        {
            const InterfacePeer &pr = iface_peers[k];
            fdd::ExchangeOp &op = iface_ops[k];
            op.peer = pr.rank;
            op.send = base + (size_t)nc * (num_bdary_nodes + pr.first);
            op.recv = base + (size_t)nc * (num_bdary_nodes + iface_shared_entries + pr.first);
            op.send_bytes = op.recv_bytes = (size_t)nc * pr.count * sizeof(double);
        }
        fdd::comm().exchange(iface_ops.data(), (int)iface_ops.size()); // every rank calls it, peers or not (one back-end meets world-wide)
    }

    void gs_add_boundary_neighbours(fdd::memory &a, fdd::memory *b)
    {
        void *stream = fdd::dev().stream;
        FDD_CALL(fdd_interface_gather(iface_buf.as<double>(), iface_gather_index.as<int>(), num_bdary_nodes + iface_shared_entries, a.as<double>(), b ? b->as<double>() : nullptr, stream));
        iface_exchange(b ? 2 : 1);
        FDD_CALL(fdd_interface_sum(a.as<double>(), b ? b->as<double>() : nullptr, iface_sum_ptr.as<int>(), iface_sum_col.as<int>(), num_bdary_nodes, iface_buf.as<double>(), stream));
    }

    void gs_add_boundary(fdd::memory &t)
    {
        if (fdd::comm().size == 1 or num_interface_slots == 0) return;
        if (neighbour_interface_exchange)
        {
            gs_add_boundary_neighbours(t, nullptr);
            return;
        }
        FDD_CALL(fdd_memset(interface_slots.ptr(), 0, (size_t)num_interface_slots * sizeof(double), fdd::dev().stream));
        FDD_CALL(fdd_interface_pack(interface_slots.as<double>(), bdary_slot.as<int>(), t.as<double>(), num_bdary_nodes, fdd::dev().stream));
        fdd::comm().allreduce_sum(interface_slots.as<double>(), num_interface_slots);
        FDD_CALL(fdd_interface_unpack(t.as<double>(), interface_slots.as<double>(), bdary_slot.as<int>(), num_bdary_nodes, fdd::dev().stream));
    }

    // two boundary prefixes in ONE exchange (one collective latency instead of two)
    void gs_add_boundary_pair(fdd::memory &a, fdd::memory &b)
    {
        if (fdd::comm().size == 1 or num_interface_slots == 0) return;
        if (neighbour_interface_exchange)
        {
            gs_add_boundary_neighbours(a, &b);
            return;
        }
        const int S = num_interface_slots;
        void *stream = fdd::dev().stream;
        FDD_CALL(fdd_memset(interface_slots.ptr(), 0, 2 * (size_t)S * sizeof(double), stream));
        FDD_CALL(fdd_interface_pack(interface_slots.as<double>(), bdary_slot.as<int>(), a.as<double>(), num_bdary_nodes, stream));
        FDD_CALL(fdd_interface_pack(interface_slots.as<double>() + S, bdary_slot.as<int>(), b.as<double>(), num_bdary_nodes, stream));
        fdd::comm().allreduce_sum(interface_slots.as<double>(), 2 * S);
        FDD_CALL(fdd_interface_unpack(a.as<double>(), interface_slots.as<double>(), bdary_slot.as<int>(), num_bdary_nodes, stream));
        FDD_CALL(fdd_interface_unpack(b.as<double>(), interface_slots.as<double>() + S, bdary_slot.as<int>(), num_bdary_nodes, stream));
    }

    // device scalars -> (all-reduce) -> host
    void fetch_scalars(DType *out, int n)
    {
        if (fdd::comm().size > 1) fdd::comm().allreduce_sum(scalars.as<double>(), n);
        scalars.copyTo(out, n * sizeof(DType));
    }

    void residual_norm(DType &r_norm, fdd::memory &r)
    {
        direct_stiffness_summation(work_dev[1], r);
        FDD_CALL(fdd_dom_residual_norm(scalars.as<double>(), reduce_ws.as<double>(), r.as<double>(), work_dev[1].as<double>(), dirichlet_mask.as<double>(), num_local_points, fdd::dev().stream));
        fetch_scalars(&r_norm, 1);
        r_norm = std::sqrt(r_norm);
    }

    void assembled_inner_product(DType &uv, fdd::memory &u, fdd::memory &v)
    {
        direct_stiffness_summation(work_dev[1], v);
        FDD_CALL(fdd_dom_inner_product(scalars.as<double>(), reduce_ws.as<double>(), u.as<double>(), work_dev[1].as<double>(), dirichlet_mask.as<double>(), num_local_points, fdd::dev().stream));
        fetch_scalars(&uv, 1);
    }

    void projection_inner_products(DType &gamma_k, DType &theta_k, fdd::memory &z, fdd::memory &r, fdd::memory &p, fdd::memory &q)
    {
        DType values[2];
        FDD_CALL(fdd_dom_projection_inner_products(scalars.as<double>(), reduce_ws.as<double>(), z.as<double>(), r.as<double>(), p.as<double>(), q.as<double>(), num_local_points, fdd::dev().stream));
        fetch_scalars(values, 2);
        gamma_k = values[0];
        theta_k = values[1];
    }

    void solution_and_residual_update(fdd::memory &u, fdd::memory &r1, fdd::memory &r, fdd::memory &p, fdd::memory &q, DType alpha_k)
    {
        FDD_CALL(fdd_dom_solution_and_residual_update(u.as<double>(), r1.as<double>(), r.as<double>(), p.as<double>(), q.as<double>(), alpha_k, num_local_points, fdd::dev().stream));
    }

    void inner_product_flexible(DType &theta_k, fdd::memory &r, fdd::memory &r1, fdd::memory &z)
    {
        FDD_CALL(fdd_dom_inner_product_flexible(scalars.as<double>(), reduce_ws.as<double>(), r.as<double>(), r1.as<double>(), z.as<double>(), num_local_points, fdd::dev().stream));
        fetch_scalars(&theta_k, 1);
    }

    void residual_and_search_update(fdd::memory &p, fdd::memory &r, fdd::memory &z, fdd::memory &r1, DType beta_k)
    {
        FDD_CALL(fdd_dom_residual_and_search_update(p.as<double>(), r.as<double>(), z.as<double>(), r1.as<double>(), beta_k, num_local_points, fdd::dev().stream));
    }

    template <typename PType>
    void apply_preconditioner(fdd::memory &z, fdd::memory &r, PType &subdomain)
    {
        if (use_preconditioner)
        {
            fdd_timer().start("subdomain.solver");
            if (preconditioner_type == 0)
                subdomain.flexible_conjugate_gradient(z, r);
            else
                subdomain.generalized_minimum_residual(z, r);
            fdd_timer().stop("subdomain.solver");

            fdd_timer().start("subdomain.stitching");
            direct_stiffness_summation(z, z, true, true);
            fdd_timer().stop("subdomain.stitching");
        }
        else
        {
            direct_stiffness_summation(z, r);
        }
    }

    // VA[i] = mask * QQt V[i], made once per basis vector (restructured outer GMRES)
    void gmres_cache_assembled(int upto)
    {
        if ((int)VA.size() != num_vectors + 1)
        {
            VA.resize(num_vectors + 1);
            for (auto &m : VA) m = fdd::dev().malloc<DType>(num_local_points);
            va_valid = 0;
        }
        for (int i = va_valid; i <= upto; i++) direct_stiffness_summation(VA[i], V[i]);
        va_valid = std::max(va_valid, upto + 1);
    }

    // The basis follows num_vectors, which fddh_problem_set_options may change between two solves.
    void allocate_gmres()
    {
        if (gmres_point_vectors == num_vectors) return;
        for (auto *set : {&V, &Z}) set->clear();
        V.resize(num_vectors + 1);
        for (int i = 0; i < num_vectors + 1; i++) V[i] = fdd::dev().malloc<DType>(num_local_points);
        Z.resize(num_vectors);
        for (int i = 0; i < num_vectors; i++) Z[i] = fdd::dev().malloc<DType>(num_local_points);
        va_valid = 0;
        gmres_point_vectors = num_vectors;
    }

    // The outer iteration is the reference's Domain loop: gmres.hpp says what the two switches stand for.
    fdd::GmresControl<DType> outer_gmres_control(bool use_relative) const { return {max_iterations, tolerance, use_relative, /* count_at_step_start */ false, /* stop_on_nan */ true}; }
    static void print_outer_step(int step, DType r_norm, DType relative) { rstdout("Iter %2d: | residual_norm = %24.16g | relative_residual_norm = %24.16g | \n", step, r_norm, relative); }

    // H[i][col] = sum q * b[i] * mask for i < count: q is read once per group of FDD_MULTI_MAX vectors
    void grouped_inner_products(std::vector<std::vector<DType>> &H, int col, fdd::memory &q, const double *const *b, int count, fdd::memory &mask, int n)
    {
        double h[FDD_MULTI_MAX];
        for (int g0 = 0; g0 < count; g0 += FDD_MULTI_MAX)
        {
            const int cnt = std::min(FDD_MULTI_MAX, count - g0);
            FDD_CALL(fdd_multi_weighted_inner_product(scalars.as<double>(), reduce_ws.as<double>(), q.as<double>(), b + g0, cnt, mask.as<double>(), n, fdd::dev().stream));
            fetch_scalars(h, cnt);
            for (int i = 0; i < cnt; i++) H[g0 + i][col] = h[i];
        }
    }

    // y += sum_{i < count} coeffs[i] * x[i], one pass over y per group of FDD_MULTI_MAX vectors
    void grouped_axpy(fdd::memory &y, const DType *coeffs, std::vector<fdd::memory> &x, int count, int n)
    {
        for (int g0 = 0; g0 < count; g0 += FDD_MULTI_MAX)
        {
            const int cnt = std::min(FDD_MULTI_MAX, count - g0);
            const double *ptrs[FDD_MULTI_MAX];
            for (int i = 0; i < cnt; i++) ptrs[i] = x[g0 + i].template as<double>();
            FDD_CALL(fdd_multi_axpy(y.as<double>(), coeffs + g0, ptrs, cnt, n, fdd::dev().stream));
        }
    }

  public:
    // Member variables (domain.hpp:94-123)
    std::string directory;
    int poly_degree = 1;
    const char *data_type = "double";

    int num_total_elements = 0;
    long long num_total_points = 0;
    long long num_total_nodes = 0; // unique global nodes (the reference never assigns it, domain.hpp:100)

    int num_local_elements = 0;
    int num_local_points = 0;
    int num_local_nodes = 0;

    int num_elem_points = 0;

    MeshData<DType> mesh;
    std::vector<Element<DType>> elements;

    // Solver
    int num_blocks = 0;
    int num_iterations = 0;
    int num_vectors = 20;
    int max_iterations = 500;
    int preconditioner_type = 1;
    bool use_preconditioner = true;
    bool fused_dssum = true; // gather-scatter kernel instead of the reference's Qt / Q SpMV pair
    bool neighbour_interface_exchange = true; // gs_add on the boundary prefix: grouped sends / receives between the sharing ranks (false: the dense interface-slot all-reduce)
    bool restructured_outer = true; // outer GMRES: cached assembled basis, multi-dot, multi-axpy
    bool assembled_outer = true; // flexible CG on node vectors (one value per assembled node) when the configuration allows it
    bool device_scalars = true;  // node-space flexible CG: alpha / beta read by the update kernels from device memory, residual norm fetched late
    bool lazy_steps = true;      // fcg_steps: K iterations with one host synchronisation at the end
    bool shared_residual_norm = true; // one rank: the outer residual norm and the inner solve's first norm are the same sum over the dof slice, formed once (the iterates keep their bits; the recorded norm groups its terms differently)
    bool early_gamma = true;      // device scalars: the flexible dot also forms the next iteration's gamma = <z, r+> (same bits; the projection kernel is left with <p, q>)
    bool fused_update_flexible_dot = true; // one rank, z~ written in place, early_gamma: the inner solve's final update of z~ is formed inside the flexible dot's pass (same bits; 0: a kernel of its own in front of the dot)
    bool fused_residual_norm = true; // one rank, the norm is the dof slice's plain sum (shared_residual_norm): r+ = r - alpha q sums the squares of what it stores (same bits; 0: the norm reads r+ back)
    bool solution_in_direction_pass = true; // device scalars: u~ += alpha p~ rides in the pass of p~ = z~ + beta p~, which loads p~ once for both (same bits; 0: in the residual update's pass)
    bool unit_stitch_in_place = true; // stitching weights of the dof slice all exactly 1 (one rank): the inner solve writes z~ in place (0: the multiplication by the ones, the reference's sequence)
    fdd::StiffnessFlags stiffness; // which kernel the element operator runs (element_operator.hpp)
    DType tolerance = 1.0e-07;
    std::vector<DType> residual_history; // what the reference prints per iteration

    // Operator
    fdd::memory D_hat;
    std::vector<double> D_hat_hst;
    fdd::memory geom_fact[NUM_GEOM_FACTS];
    fdd::FieldGeometry field_geometry; // device copy of mesh.x / y / z and the GLL weights for the field operators (field_ops.hpp): made at first use, freed with the Domain

    Domain() {}
    Domain(char *directory_, int poly_degree_) { initialize(directory_, poly_degree_); }

    int boundary_nodes_count() const { return num_bdary_nodes; }
    int interface_slots_count() const { return num_interface_slots; }
    // one interface exchange of `vectors` (1 or 2) prefixes, as gs_add_boundary[_pair] issues it: the collective alone,
    // on the exchange buffer's current contents (bench.py's communication timings)
    void comm_probe_interface(int vectors, bool neighbours)
    {
        if (fdd::comm().size == 1 or num_interface_slots == 0) return;
        if (neighbours)
            iface_exchange(vectors == 2 ? 2 : 1);
        else
            fdd::comm().allreduce_sum(interface_slots.as<double>(), (size_t)num_interface_slots * (vectors == 2 ? 2 : 1));
    }
    // bytes this rank sends in one neighbour exchange of `vectors` prefixes
    double comm_interface_neighbour_bytes(int vectors) const { return (double)vectors * iface_shared_entries * sizeof(double); }
    CSR_Matrix<DType> &gather_matrix() { return Qt; }
    CSR_Matrix<DType> &scatter_matrix() { return Q; }
    fdd::memory &dirichlet_mask_memory() { return dirichlet_mask; }
    fdd::memory &assembled_weight_memory() { return assembled_weight; }

    // ---- mesh files: the format Domain::initialize reads (domain.tpp:45-224) ----
    static bool read_mesh_files(const char *dir, int poly_degree, int proc_id, MeshData<DType> &m)
    {
        char file_name[4096];
        int n_x, n_y, n_z;
        snprintf(file_name, sizeof(file_name), "%s/lx1_%d/size_%d.%d.dat", dir, poly_degree + 1, proc_id, poly_degree);
        FILE *fp = fopen(file_name, "r");
        if (!fp) return false;
        int got = fscanf(fp, "%d %d %d %d %d", &m.dim, &n_x, &n_y, &n_z, &m.num_local_elements);
        fclose(fp);
        if (got != 5) return false;
        m.poly_degree = poly_degree;
        const size_t P = (size_t)m.num_local_points();

        auto read_bin = [&](const char *stem, void *dst, size_t elem_size) -> bool {
            snprintf(file_name, sizeof(file_name), "%s/lx1_%d/%s_%d.%d.dat", dir, poly_degree + 1, stem, proc_id, poly_degree);
            FILE *f = fopen(file_name, "rb");
            if (!f) return false;
            size_t rd = fread(dst, elem_size, P, f);
            fclose(f);
            return rd == P;
        };

        bool ok = true;
        m.x.resize(P);
        ok = ok && read_bin("x", m.x.data(), sizeof(DType));
        if (m.dim >= 2)
        {
            m.y.resize(P);
            ok = ok && read_bin("y", m.y.data(), sizeof(DType));
        }
        if (m.dim >= 3)
        {
            m.z.resize(P);
            ok = ok && read_bin("z", m.z.data(), sizeof(DType));
        }
        m.glo_num.resize(P);
        ok = ok && read_bin("glo_num", m.glo_num.data(), sizeof(long long));
        m.node_degree.resize(P);
        ok = ok && read_bin("node_degree", m.node_degree.data(), sizeof(int));
        m.p_mask.resize(P);
        ok = ok && read_bin("p_mask", m.p_mask.data(), sizeof(DType));
        for (int g = 0; g < NUM_GEOM_FACTS; g++)
        {
            char stem[16];
            snprintf(stem, sizeof(stem), "g_%d", g + 1);
            m.g[g].resize(P);
            ok = ok && read_bin(stem, m.g[g].data(), sizeof(DType));
        }
        return ok;
    }

    static bool write_mesh_files(const char *dir, int proc_id, const MeshData<DType> &m)
    {
        char file_name[4096];
        const int N = m.poly_degree;
        const size_t P = (size_t)m.num_local_points();
        snprintf(file_name, sizeof(file_name), "%s/lx1_%d/size_%d.%d.dat", dir, N + 1, proc_id, N);
        FILE *fp = fopen(file_name, "w");
        if (!fp) return false;
        fprintf(fp, "%d %d %d %d %d\n", m.dim, N + 1, N + 1, (m.dim == 3) ? N + 1 : 1, m.num_local_elements);
        fclose(fp);
        auto write_bin = [&](const char *stem, const void *src, size_t elem_size) -> bool {
            snprintf(file_name, sizeof(file_name), "%s/lx1_%d/%s_%d.%d.dat", dir, N + 1, stem, proc_id, N);
            FILE *f = fopen(file_name, "wb");
            if (!f) return false;
            size_t wr = fwrite(src, elem_size, P, f);
            fclose(f);
            return wr == P;
        };
        bool ok = write_bin("x", m.x.data(), sizeof(DType));
        if (m.dim >= 2) ok = ok && write_bin("y", m.y.data(), sizeof(DType));
        if (m.dim >= 3) ok = ok && write_bin("z", m.z.data(), sizeof(DType));
        ok = ok && write_bin("glo_num", m.glo_num.data(), sizeof(long long));
        ok = ok && write_bin("node_degree", m.node_degree.data(), sizeof(int));
        ok = ok && write_bin("p_mask", m.p_mask.data(), sizeof(DType));
        for (int g = 0; g < NUM_GEOM_FACTS; g++)
        {
            char stem[16];
            snprintf(stem, sizeof(stem), "g_%d", g + 1);
            ok = ok && write_bin(stem, m.g[g].data(), sizeof(DType));
        }
        return ok;
    }

    void initialize(char *directory_, int poly_degree_)
    {
        directory = directory_;
        MeshData<DType> m;
        if (!read_mesh_files(directory_, poly_degree_, fdd::globals().proc_id, m))
        {
            pstdout("ERROR: There was a problem reading Nek5000 data\n");
            fprintf(stderr, "ERROR: There was a problem reading Nek5000 data in '%s' (lx1_%d)\n", directory_, poly_degree_ + 1);
            exit(EXIT_FAILURE);
        }
        initialize(std::move(m));
    }

    void initialize(MeshData<DType> mesh_)
    {
        mesh = std::move(mesh_);
        poly_degree = mesh.poly_degree;
        list = fdd::LevelList();
        fdd::SetupTimer timing("Domain::initialize", fdd::comm().rank == 0);
        fdd::globals().dim = mesh.dim; // `dim` is a global set by the last mesh read (config.hpp:48)
        const int dim = mesh.dim;

        num_local_elements = mesh.num_local_elements;
        num_elem_points = mesh.num_elem_points();
        num_local_points = num_local_elements * num_elem_points;

        {
            double tot = (double)num_local_elements; // domain.tpp:49-50
            fdd::comm().allreduce_sum_host(&tot, 1);
            num_total_elements = (int)std::llround(tot);
            mesh.num_total_elements = num_total_elements;
            num_total_points = (long long)num_total_elements * num_elem_points;
        }

        // Work arrays
        work_dev.resize(3);
        for (int w = 0; w < 3; w++) work_dev[w] = fdd::dev().malloc<DType>(num_local_points);

        // Elements (light views)
        elements.clear();
        elements.reserve(num_local_elements);
        for (int e = 0; e < num_local_elements; e++)
        {
            elements.push_back(Element<DType>(e, dim, poly_degree));
            elements.back().bind(mesh);
        }

        dirichlet_mask = fdd::dev().malloc<DType>(num_local_points);
        dirichlet_mask.copyFrom(mesh.p_mask.data(), (size_t)num_local_points * sizeof(DType));

        for (int g = 0; g < NUM_GEOM_FACTS; g++)
        {
            geom_fact[g] = fdd::dev().malloc<DType>(num_local_points);
            geom_fact[g].copyFrom(mesh.g[g].data(), (size_t)num_local_points * sizeof(DType));
            list.G[g] = geom_fact[g].as<double>();
        }

        timing.lap("elements, mask and factors to the device");
        // ---- communication / local numbering (domain.tpp:233-302) ----
        rstdout("Setting up domain stitching handle...\n");

        // One hash pass turns the 64-bit global ids into dense temporary ids (first appearance); the multiplicity
        // count, the four numbering passes and Q then work on plain arrays (the seven hash lookups per point of
        // the straightforward form were 40 of the 50 s of setup at N = 15).
        std::vector<int> tid(num_local_points);
        int num_tmp = 0;
        num_tmp = fdd::first_appearance_ids(mesh.glo_num.data(), (size_t)num_local_points, tid);
        timing.lap("temporary node ids");
        std::vector<int> local_node_degree(num_tmp, 0);
        for (int p = 0; p < num_local_points; p++) local_node_degree[tid[p]]++;

        std::vector<int> local_node_idx(num_tmp, -1);
        std::vector<long long> boundary_nodes;
        int count = 0;

        // Nodes whose local multiplicity differs from the global one (shared with other ranks) come first
        // (domain.tpp:249-281), the rest after them by first appearance.  Within that, Dirichlet nodes are moved to
        // the two ends -- shared Dirichlet | shared | interior | interior Dirichlet -- so that the Subdomain's dofs
        // (the unmasked nodes, in this order) are one contiguous slice of every node vector and the outer solve hands
        // its residual to the inner solve, and takes the correction back, without renumbering.  Nothing outside the
        // class sees the order except through Q / Qt.
        for (int pass = 0; pass < 4; pass++)
        {
            const bool want_shared = pass < 2;
            const bool want_dirichlet = (pass == 0 or pass == 3);
            for (int p = 0; p < num_local_points; p++)
            {
                const int t = tid[p];
                const bool shared = local_node_degree[t] != mesh.node_degree[p];
                const bool dirichlet = not(mesh.p_mask[p] > 0.0);
                if (shared != want_shared or dirichlet != want_dirichlet) continue;
                if (local_node_idx[t] < 0)
                {
                    if (shared) boundary_nodes.push_back(mesh.glo_num[p]);
                    local_node_idx[t] = count;
                    count++;
                }
            }
            if (pass == 1) num_bdary_nodes = count;
        }

        num_local_nodes = num_tmp;
        timing.lap("node numbering");

        // gs_setup (domain.tpp:283-284): dense interface slots shared by all ranks
        {
            std::vector<int> counts;
            std::vector<long long> all = fdd::comm().allgatherv_host(boundary_nodes, counts);
            if (fdd::comm().size > 1) build_interface_neighbour_plan(all, counts, boundary_nodes);
            std::sort(all.begin(), all.end());
            all.erase(std::unique(all.begin(), all.end()), all.end());
            num_interface_slots = (int)all.size();

            if (num_bdary_nodes > 0)
            {
                std::vector<int> slot(num_bdary_nodes);
                for (int b = 0; b < num_bdary_nodes; b++) slot[b] = (int)(std::lower_bound(all.begin(), all.end(), boundary_nodes[b]) - all.begin());
                bdary_slot = fdd::dev().malloc<int>(num_bdary_nodes);
                bdary_slot.copyFrom(slot.data(), (size_t)num_bdary_nodes * sizeof(int));
            }
            if (num_interface_slots > 0) interface_slots = fdd::dev().malloc<double>(2 * (size_t)num_interface_slots); // room for two prefixes in one exchange

            // unique global nodes = sum of owned nodes: interior ones + shared ones counted once
            double owned = (double)(num_local_nodes - num_bdary_nodes);
            fdd::comm().allreduce_sum_host(&owned, 1);
            num_total_nodes = (long long)std::llround(owned) + num_interface_slots;
        }

        timing.lap("interface slots");
        {
            // one unit entry per point, rows in order: what add_entry + assemble (domain.tpp:286-296) produce, written directly
            std::vector<int> q_ptr((size_t)num_local_points + 1);
            fdd::low_order::pod_vector<int> q_col((size_t)num_local_points);
            fdd::low_order::pod_vector<DType> q_val((size_t)num_local_points);
            fdd::low_order::parallel_ranges(num_local_points, fdd::low_order::range_parts(num_local_points), [&](long long p0, long long p1, int) {
                for (long long p = p0; p < p1; p++)
                {
                    q_ptr[p] = (int)p;
                    q_col[p] = local_node_idx[tid[p]];
                    q_val[p] = (DType)1.0;
                }
            });
            q_ptr[num_local_points] = num_local_points;
            Q.adopt_csr(num_local_points, num_local_nodes, std::move(q_ptr), std::move(q_col), std::move(q_val));
        }
        timing.lap("Q");
        Q.transpose(Qt);
        timing.lap("Qt");

        reduce_ws = fdd::dev().malloc<double>(fdd_reduce_workspace_doubles());
        scalars = fdd::dev().malloc<double>(8);

        assembled_weight = fdd::dev().malloc<DType>(num_local_nodes);
        math.set_to_value(work_dev[0], 1.0, num_local_points);
        Qt.multiply(assembled_weight, work_dev[0]);
        gs_add_boundary(assembled_weight);
        math.invert_vector_elements(assembled_weight, num_local_nodes);

        // Operator (domain.tpp:304-316)
        const int n = poly_degree + 1;
        std::vector<double> r_gll(n), w_gll(n);
        D_hat_hst.assign((size_t)n * n, 0.0);
        fdd::gll::zwgll(r_gll.data(), w_gll.data(), n);
        fdd::gll::dgll(D_hat_hst.data(), r_gll.data(), n);
        D_hat = fdd::dev().malloc<DType>((size_t)n * n);
        D_hat.copyFrom(D_hat_hst.data(), (size_t)n * n * sizeof(DType));
        list.poly_degree = poly_degree;
        list.dim = dim;
        list.num_elements = num_local_elements;
        list.D_hat = D_hat.as<double>(); // set_D_hat rewrites this buffer in place
        fdd::detect_zero_factors(list); // the list is complete: are its off-diagonal factor arrays zero everywhere?
        fdd::detect_shared_blocks(list); // and do its elements share their factor blocks?
        fdd::check_lean_table(list, D_hat_hst); // and does the table uploaded above allow the lean line instance?

        // Solver vectors (GMRES bases are allocated on first use)
        r_k = fdd::dev().malloc<DType>(num_local_points);
        r_kp1 = fdd::dev().malloc<DType>(num_local_points);
        q_k = fdd::dev().malloc<DType>(num_local_points);
        z_k = fdd::dev().malloc<DType>(num_local_points);
        p_k = fdd::dev().malloc<DType>(num_local_points);

        num_blocks = (num_local_points + BLOCK_SIZE - 1) / BLOCK_SIZE;
    }

    // Replace D_hat (tests feed the reference's own table so that parity does
    // not depend on the last bits of the GLL nodes)
    void set_D_hat(const double *D, int n)
    {
        D_hat_hst.assign(D, D + (size_t)n * n);
        D_hat.copyFrom(D_hat_hst.data(), (size_t)n * n * sizeof(DType));
        fdd::check_lean_table(list, D_hat_hst);
    }

    // domain.tpp:527-580
    void initial_function(fdd::memory &u, int function_id = 0, unsigned long long seed = 0)
    {
        std::vector<DType> w(num_local_points);
        const int dim = mesh.dim;
        // function_id 3/4 use rand()/RAND_MAX in the reference, unseeded
        // (domain.tpp:572-573); srand(seed) makes runs repeatable
        if (function_id == 3 or function_id == 4) srand((unsigned)seed);
        for (int p = 0; p < num_local_points; p++)
        {
            const DType x = mesh.x[p], y = mesh.y[p], z = (dim == 3) ? mesh.z[p] : 0.5;
            const DType sz = (dim == 3) ? std::sin(M_PI * z) : 1.0;
            DType v = 0.0;
            if (function_id == 0)
                v = std::sin(M_PI * x) * std::sin(M_PI * y) * sz;
            else if (function_id == 1)
                v = std::sin(M_PI * x) * std::sin(M_PI * y) * sz + std::sin(2.0 * M_PI * x) * std::sin(M_PI * y) * sz;
            else if (function_id == 2)
                v = std::exp(x) * std::sin(M_PI * x) * std::sin(M_PI * y) * sz;
            else if (function_id == 3)
                v = std::sin(M_PI * x) * std::sin(M_PI * y) * sz + (1.0 / 5.0) * ((DType)(rand()) / (DType)(RAND_MAX));
            else if (function_id == 4)
                v = (DType)(rand()) / (DType)(RAND_MAX);
            w[p] = v;
        }
        u.copyFrom(w.data(), (size_t)num_local_points * sizeof(DType));
        direct_stiffness_summation(u, u, true, true);
    }

    // domain.tpp:582-600
    void direct_stiffness_summation(fdd::memory &QQtu, fdd::memory &u, bool apply_dirichlet_mask = true, bool apply_assembled_weight = false)
    {
        if (fused_dssum and Qt.unit_values)
        {
            // One gather-scatter pass over the assembled nodes instead of the
            // Qt and Q SpMVs (same arithmetic, bit-identical; fdd_hip.h).  The
            // boundary prefix is gathered first, exchanged, and scattered last.
            const double *w = apply_assembled_weight ? assembled_weight.as<double>() : nullptr;
            const double *m = apply_dirichlet_mask ? dirichlet_mask.as<double>() : nullptr;
            // every rank of a multi-rank run enters the exchange, also one without shared nodes (an empty prefix):
            // the collectives must match across ranks (gs_add_boundary and node_norm_enqueue gate the same way)
            const bool multi = fdd::comm().size > 1 and num_interface_slots > 0;
            const int nb = multi ? num_bdary_nodes : 0;
            if (multi)
            {
                if (nb > 0) Qt.gather_scatter(nullptr, work_dev[0].as<double>(), u.as<double>(), w, nullptr, 0, nb, 1);
                gs_add_boundary(work_dev[0]);
            }
            Qt.gather_scatter(QQtu.as<double>(), nullptr, u.as<double>(), w, m, nb, num_local_nodes, 0);
            if (nb > 0) Qt.gather_scatter(QQtu.as<double>(), work_dev[0].as<double>(), nullptr, nullptr, m, 0, nb, 2);
            return;
        }

        if (apply_assembled_weight)
            Qt.multiply_weight(work_dev[0], u, assembled_weight);
        else
            Qt.multiply(work_dev[0], u);

        gs_add_boundary(work_dev[0]);

        if (apply_dirichlet_mask)
            Q.multiply_weight(QQtu, work_dev[0], dirichlet_mask);
        else
            Q.multiply(QQtu, work_dev[0]);
    }

    // domain.tpp:602-609
    void stiffness_matrix(fdd::memory &Au, fdd::memory &u, bool apply_dssum = false)
    {
        fdd::apply_local(list, Au.as<double>(), u.as<double>(), work_dev, stiffness);
        if (apply_dssum) direct_stiffness_summation(Au, Au, true, false);
    }

    // ------------------------------------------------------------------
    // Flexible CG on assembled data.  The reference keeps every Krylov vector
    // per element-local point, but its recurrences only ever combine
    //   - continuous vectors (u, p, z: the same value on every copy of a node),
    //   - residual-type vectors (r, q) that enter through point-wise dots with
    //     continuous vectors, sum_p z_p r_p = sum_n z_n (Qt r)_n, through the
    //     residual norm <r, QQt r>, and through the preconditioner, which
    //     starts with Qt (subdomain.tpp:3996) itself.
    // So the iteration is carried on node vectors: u~, p~, z~ (one value per
    // node) and r^ = Qt r, q^ = Qt q (this rank's partial sums).  Per step: the
    // element stiffness reads Q p~ through the point -> node index array, one
    // gather Qt, and everything else is BLAS-1 on num_local_nodes values (0.68x
    // the points at N = 7) with no dssum pass; the inner solve takes r^ and
    // returns u~ directly in the subdomain's dof numbering.  Interface nodes
    // (the boundary prefix) are exchanged exactly where the reference's gs_op
    // sits: inside the residual norm and in the stitching.
    // Same recurrences as domain.tpp:611-725; iterates agree to rounding.
    // ------------------------------------------------------------------
    template <typename PType>
    bool can_fcg_nodes(PType &subdomain)
    {
        if (not(assembled_outer and Qt.unit_values and mesh.dim == 3 and poly_degree <= 15)) return false;
        if (not use_preconditioner) return true;
        if (preconditioner_type != 1 and not subdomain.chebyshev()) return false; // the Chebyshev-Jacobi inner solve stands in for either Krylov solve
        if (subdomain.composite()) return subdomain.composite_dof_space() and own_nodes_have_dofs(subdomain);
        return subdomain.assembled_inner and subdomain.can_assemble() and (int)subdomain.point_dof.size() == num_local_points;
    }

    // composite region: every unmasked node of the rank carries one of the subdomain's leading (own) dofs -- always,
    // unless the region has no ring at the rank's own degree (subdomain_overlap 0), where own points hang
    template <typename PType>
    bool own_nodes_have_dofs(PType &subdomain)
    {
        const int nd = subdomain.own_dofs();
        for (int p = 0; p < num_local_points; p++)
        {
            const int d = subdomain.point_dof[p];
            if (mesh.p_mask[p] > 0.0 and (d < 0 or d >= nd)) return false;
        }
        return true;
    }

    void setup_nodes()
    {
        if (nodes_ready) return;
        const int nn = num_local_nodes;
        point_node_dev = fdd::dev().malloc<int>(std::max(num_local_points, 1));
        point_node_dev.copyFrom(Q.col_hst.data(), (size_t)num_local_points * sizeof(int)); // one entry per row of Q

        std::vector<DType> mask(nn, 1.0), stitch(nn), w(nn);
        for (int p = 0; p < num_local_points; p++) mask[Q.col_hst[p]] = mesh.p_mask[p];
        assembled_weight.copyTo(w.data(), (size_t)nn * sizeof(DType));
        for (int n = 0; n < nn; n++) stitch[n] = (DType)(Qt.ptr_hst[n + 1] - Qt.ptr_hst[n]) * w[n] * mask[n];
        node_mask = fdd::dev().malloc<DType>(std::max(nn, 1));
        node_mask.copyFrom(mask.data(), (size_t)nn * sizeof(DType));
        node_stitch = fdd::dev().malloc<DType>(std::max(nn, 1));
        node_stitch.copyFrom(stitch.data(), (size_t)nn * sizeof(DType));
        node_stitch_hst = stitch;
        node_mask_hst = mask;

        for (fdd::memory *v : {&nu, &nr, &nr1, &nq, &nz, &np, &nt}) *v = fdd::dev().malloc<DType>(std::max(nn, 1));
        nodes_ready = true;
    }

    template <typename PType>
    void setup_dof_maps(PType &subdomain)
    {
        // the dofs that sit on this rank's nodes: all of them for an own-elements region, the leading ones of a composite
        const int nd = subdomain.own_dofs();
        if (nodes_sub_dofs == nd and node_of_dof.ptr()) return;
        composite_precond = subdomain.composite();
        std::vector<int> n_of_d(std::max(nd, 1), -1), d_of_n(std::max(num_local_nodes, 1), -1);
        for (int p = 0; p < num_local_points; p++)
        {
            const int d = subdomain.point_dof[p];
            if (d >= 0 and d < nd)
            {
                n_of_d[d] = Q.col_hst[p];
                d_of_n[Q.col_hst[p]] = d;
            }
        }
        dof_shift = (nd > 0) ? n_of_d[0] : -1;
        for (int d = 0; d < nd and dof_shift >= 0; d++)
            if (n_of_d[d] != d + dof_shift) dof_shift = -1;
        if (dof_shift > 0 and (dof_shift & 1)) dof_shift = -1; // an odd shift would leave the slice 8-byte aligned only: the 16-byte kernels want more
        node_of_dof = fdd::dev().malloc<int>(std::max(nd, 1));
        node_of_dof.copyFrom(n_of_d.data(), (size_t)nd * sizeof(int));
        dof_of_node = fdd::dev().malloc<int>(std::max(num_local_nodes, 1));
        dof_of_node.copyFrom(d_of_n.data(), (size_t)num_local_nodes * sizeof(int));
        sub_f = fdd::dev().malloc<DType>(std::max(nd, 1));
        sub_u = subdomain.new_dof_vector(); // a composite keeps copies / hanging values behind its dofs
        if (composite_precond and not rp.ptr()) rp = subdomain.tree_points(); // lives in the Subdomain's tree vector: level 0 is read in place
        nodes_sub_dofs = nd;
        norm_on_dof_slice = fdd::comm().size == 1 and dof_shift >= 0 and not composite_precond and subdomain.unit_norm_weight() and (int)node_mask_hst.size() == num_local_nodes;
        for (int n = 0; n < num_local_nodes and norm_on_dof_slice; n++)
            if (node_mask_hst[n] != ((n >= dof_shift and n < dof_shift + nd) ? (DType)1.0 : (DType)0.0)) norm_on_dof_slice = false;
        stitch_is_one = dof_shift >= 0 and not composite_precond and (int)node_stitch_hst.size() >= dof_shift + nd;
        for (int d = 0; d < nd and stitch_is_one; d++)
            if (node_stitch_hst[(size_t)dof_shift + d] != (DType)1.0) stitch_is_one = false;
    }

    // t = Qt v: this rank's sums over the copies of every node (no exchange)
    void gather_nodes(fdd::memory &t, fdd::memory &v)
    {
        Qt.gather_scatter(nullptr, t.as<double>(), v.as<double>(), nullptr, nullptr, 0, num_local_nodes, 1);
    }

    // ---- affine elements (an option of this build, element_operator.hpp) ----
    // set_affine_geometry(true) switches the node-space operator over only if every element of the mesh passes the check
    // (a box mesh); false: it did not, or the mesh cannot run that kernel.
    const fdd::LevelList &operator_list() const { return list; }
    fdd::StiffnessChoice operator_choice() const { return fdd::choose_stiffness(list, stiffness, false, fdd::StiffnessForm::gather); } // what the fddh_problem_*_info entries report
    bool set_affine_geometry(bool on)
    {
        list.affine_requested = on;
        list.affine = on and fdd::detect_affine(list);
        return list.affine or not on;
    }

    // ---- a diffusivity per point: -div(kappa grad u), diffusivity.hpp -- a LABELLED OPTION of this build ----
    // kappa over the fine level's points (the caller has checked it, fdd::diffusivity::refusal); nullptr clears.  The scaled
    // arrays G' = mesh.g * kappa go into the buffers the list -- and the Subdomain's level-0 list, which aliases them -- already
    // reads, what is derived from a list's arrays is derived again, and a list whose unscaled blocks repeat gets the members of
    // the coefficient line instance.  mesh.g is never written: setting again or clearing starts from it.  The caller tells
    // the Subdomain (Subdomain::set_diffusivity) and ends in the C API's operator_changed.
    bool diffusivity_is_set = false; // the Subdomain keeps the values (its hierarchy is built from them)
    fdd::diffusivity::UnscaledBlocks unscaled_blocks;
    bool diffusivity_active() const { return diffusivity_is_set; }
    void set_diffusivity(const DType *kappa)
    {
        if (kappa == nullptr and not diffusivity_active()) return;
        unscaled_blocks.remember(list); // the first time: the list's arrays are still the mesh's own
        diffusivity_is_set = kappa != nullptr;
        for (int g = 0; g < NUM_GEOM_FACTS; g++) fdd::diffusivity::upload_scaled(geom_fact[g], mesh.g[g], kappa);
        fdd::diffusivity::refresh_list(list);
        const std::vector<DType> *g[3] = {&mesh.g[0], &mesh.g[1], &mesh.g[2]};
        fdd::diffusivity::fill_coef(list, unscaled_blocks, kappa, g);
    }

    // q (points) = A_local (Q p~)
    void stiffness_from_nodes(fdd::memory &q, fdd::memory &pn)
    {
        fdd::apply_gather(list, q.as<double>(), pn.as<double>(), point_node_dev.as<int>(), nullptr, num_local_nodes, stiffness);
    }

    // ---- Helmholtz shift: the node-space outer operator is Qt A_L Q + diag(c) -- a LABELLED OPTION of this build ----
    // c[n] = sum over the copies p of node n of lambda_p B_p (B: the diagonal mass matrix, fdd_field_mass): the products in
    // double on the host, summed in the column order of Qt's row.  Like r^ and q^ it is this rank's partial sum; p~ is
    // continuous, so q^ += c .* p~ behind the gather is the whole term (one rank: the C API refuses the others).  Not inside
    // the stiffness kernels: there the term would be lambda_p B_p u_p per point, two more streams in the kernel that is
    // closest to its register and LDS limits, in every instance of it; on the assembled vectors it is one stream and no
    // stiffness kernel changes.  lambda_B == nullptr or all zero: off.
    // A c that is zero on most nodes (a Robin term alone: boundary.hpp) is also kept compressed, and the pass that only adds
    // the term runs on its support (flag "indexed_shift"); the fused shift-and-dot reads both vectors anyway and stays.
    std::vector<DType> shift_nodes_hst;
    fdd::memory shift_nodes;
    fdd::boundary::ShiftSupport shift_support;
    bool indexed_shift = fdd::missing_indexed_shift_entry() == nullptr; // on where the entries are: measured faster
    bool shift_indexed() const { return shift_active() and shift_support.applies(indexed_shift, num_local_nodes); }
    bool shift_active() const { return not shift_nodes_hst.empty(); }
    void set_shift(const DType *lambda_B)
    {
        shift_nodes = fdd::memory();
        shift_nodes_hst.clear();
        shift_support.release();
        if (lambda_B == nullptr) return;
        std::vector<DType> c((size_t)num_local_nodes, 0.0);
        bool any = false;
        for (int n = 0; n < num_local_nodes; n++)
        {
            DType s = 0.0;
            for (int t = Qt.ptr_hst[n]; t < Qt.ptr_hst[n + 1]; t++) s += lambda_B[Qt.col_hst[t]];
            c[n] = s;
            any = any or s != 0.0;
        }
        if (not any) return;
        shift_nodes_hst = std::move(c);
        shift_nodes = fdd::dev().malloc<DType>(shift_nodes_hst.size());
        shift_nodes.copyFrom(shift_nodes_hst.data(), shift_nodes_hst.size() * sizeof(DType));
        shift_support.build(shift_nodes_hst);
    }
    // q^ += c .* p~ behind stiffness_from_nodes + gather_nodes
    void shift_add_nodes(fdd::memory &qn, fdd::memory &pn)
    {
        if (shift_indexed())
            fdd::ops::shift_add_indexed(qn.as<double>(), shift_support.values.as<double>(), shift_support.index.as<int>(), shift_support.count, nullptr, pn.as<double>(), num_local_nodes, fdd::dev().stream);
        else if (shift_active())
            FDD_CALL(fdd_shift_add(qn.as<double>(), shift_nodes.as<double>(), nullptr, pn.as<double>(), num_local_nodes, fdd::dev().stream));
    }

    // q^ = (Qt A_L Q + diag(c)) v~ on the caller's node vectors and <v~, q^>: the launches of fcg_nodes_step_residual's
    // operator application and of the dot behind it, in their order (a test sees what the outer step computes)
    DType node_operator(fdd::memory &qn, fdd::memory &vn)
    {
        setup_nodes();
        fcg_flush_solution_update(); // a stepwise solve in progress may still owe an update whose alpha sits in the slot written below
        void *stream = fdd::dev().stream;
        double *out = scalars.as<double>() + SLOT_PQ;
        stiffness_from_nodes(q_k, vn);
        gather_nodes(qn, q_k);
        if (shift_active())
            FDD_CALL(fdd_shift_add_inner_product(out, reduce_ws.as<double>(), qn.as<double>(), shift_nodes.as<double>(), vn.as<double>(), num_local_nodes, stream));
        else
            FDD_CALL(fdd_sub_inner_product(out, reduce_ws.as<double>(), vn.as<double>(), qn.as<double>(), num_local_nodes, stream));
        DType vq = 0.0;
        scalars.slice(SLOT_PQ, 1).copyTo(&vq, sizeof(DType));
        return vq;
    }

    // whether node_norm_enqueue forms the norm as the plain sum over the dof slice (and returns its address)
    bool norm_is_slice_sum() const
    {
        const bool multi = fdd::comm().size > 1 and num_interface_slots > 0;
        // (only with the inner solve to share it with: without a preconditioner the norm keeps its masked form, whether or not
        // an earlier solve of this problem set the dof maps up)
        return not multi and norm_on_dof_slice and shared_residual_norm and use_preconditioner;
    }

    // sqrt(<r, QQt r>) (domain.tpp:916-931) from r^ = Qt r: sum_n r^_n * gs(r^)_n * mask_n.
    // Two halves: the reductions (+ all-reduce) are enqueued into scalars[SLOT_NORM..]; the value is
    // fetched when the host wants it, which may be after more work has been enqueued.
    // defer_exchange: the boundary prefix is only saved; its exchange rides with the stitching exchange of the
    // preconditioner that follows (precondition_nodes), which then finishes the norm (node_norm_finish)
    // Returns the device address of |r^ restricted to the dof slice|^2 when -- and only when -- the sum just enqueued IS that
    // number (one rank, shared_residual_norm): the caller hands it to the precondition_nodes call that receives the same,
    // unmodified rn (the inner solve's first norm); every other branch returns nullptr.
    const double *node_norm_enqueue(fdd::memory &rn, bool defer_exchange = false)
    {
        const int nn = num_local_nodes;
        // every rank of a multi-rank run takes the two-part path (a rank without shared nodes contributes an empty
        // prefix), so that all of them issue the same collectives
        const bool multi = fdd::comm().size > 1 and num_interface_slots > 0;
        const int nb = multi ? num_bdary_nodes : 0;
        double *out = scalars.as<double>() + SLOT_NORM;
        if (multi)
        {
            if (not nprefix.ptr()) nprefix = fdd::dev().malloc<DType>(std::max(num_bdary_nodes, 1));
            nprefix.copyFrom(rn, (size_t)nb * sizeof(DType));
            FDD_CALL(fdd_dom_residual_norm(out + 1, reduce_ws.as<double>(), rn.as<double>() + nb, rn.as<double>() + nb, node_mask.as<double>() + nb, nn - nb, fdd::dev().stream));
            norm_state.parts = 2;
            norm_state.source = rn.as<double>();
            if (defer_exchange)
            {
                norm_state.deferred = true;
                return nullptr;
            }
            gs_add_boundary(nprefix);
            node_norm_finish();
            return nullptr;
        }
        const double *known = nullptr;
        if (norm_is_slice_sum())
        {
            // One rank, mask = 1 on the dof slice and 0 elsewhere: the masked sum over the nodes IS the plain sum over the
            // slice -- the sum the inner solve forms first (its right-hand side is this slice, read in place).  Formed once,
            // by the inner solve's own call, and handed to it (precondition_nodes): the iterates keep their bits, the
            // recorded norm differs from the masked form in how its terms are grouped.
            const double *self[1] = {rn.as<double>() + dof_shift};
            FDD_CALL(fdd_multi_weighted_inner_product_scaled(out, reduce_ws.as<double>(), self[0], self, nullptr, 1, nullptr, nodes_sub_dofs, fdd::dev().stream));
            known = out;
        }
        else
        {
            // sum r*r*mask with r read once (the arithmetic and the reduction tree of residual_norm_kernel, domain.okl:109-138)
            const double *self[1] = {rn.as<double>()};
            FDD_CALL(fdd_multi_weighted_inner_product(out, reduce_ws.as<double>(), rn.as<double>(), self, 1, node_mask.as<double>(), nn, fdd::dev().stream));
        }
        norm_state.parts = 1;
        if (fdd::comm().size > 1) fdd::comm().allreduce_sum(out, norm_state.parts);
        return known;
    }

    // rn1 = rn - (*num / *den) qn with node_norm_enqueue(rn1)'s slice sum formed from the values as they are stored (flag
    // "fused_residual_norm"): that call's sum to the bit, without its pass over rn1.  Only where norm_is_slice_sum().
    const double *residual_update_and_norm_enqueue(fdd::memory &rn1, fdd::memory &rn, fdd::memory &qn, const double *num, const double *den)
    {
        const int nn = num_local_nodes;
        double *out = scalars.as<double>() + SLOT_NORM;
        fdd::ProfileScope prof("residual_update_norm_kernel", 24.0 * nn);
        FDD_CALL(fdd_dom_residual_update_norm2_dev(out, reduce_ws.as<double>(), rn1.as<double>(), rn.as<double>(), qn.as<double>(), num, den, nn, dof_shift, nodes_sub_dofs, fdd::dev().stream));
        norm_state.parts = 1;
        return out;
    }

    // the boundary part of the norm once the saved prefix has been exchanged, then the all-reduce of both parts
    void node_norm_finish()
    {
        double *out = scalars.as<double>() + SLOT_NORM;
        FDD_CALL(fdd_dom_residual_norm(out, reduce_ws.as<double>(), norm_state.source, nprefix.as<double>(), node_mask.as<double>(), num_bdary_nodes, fdd::dev().stream));
        if (norm_state.deferred and device_scalars)
            norm_state.reduce_pending = true; // its two scalars join the all-reduce of the flexible dot (fcg_nodes_step_direction)
        else
            fdd::comm().allreduce_sum(out, 2);
        norm_state.deferred = false;
    }

    DType node_norm_fetch()
    {
        DType v[2] = {0.0, 0.0};
        fdd::memory tail = scalars.slice(SLOT_NORM, 2);
        tail.copyTo(v, norm_state.parts * sizeof(DType));
        return std::sqrt(v[0] + v[1]);
    }

    const double *node_norm(DType &r_norm, fdd::memory &rn)
    {
        const double *known = node_norm_enqueue(rn);
        r_norm = node_norm_fetch();
        return known;
    }

    // z~ = M^-1 r^ and the stitching (domain.tpp:639-645, 697-706)
    // hints.known_rhs_norm2: device address of |rn's dof slice|^2 if the caller has just formed it from this very rn
    // (node_norm_enqueue's return value), else nullptr
    // hints.defer_into: the caller reads zn next in a pass of its own and can form the inner solve's final update there: where
    // the inner solve agrees (defer_into->active on return) zn's dof slice is still to be written
    template <typename PType>
    void precondition_nodes(fdd::memory &zn, fdd::memory &rn, PType &subdomain, const fdd::InnerSolveHints &hints = {})
    {
        void *stream = fdd::dev().stream;
        fdd::InnerSolveHints inner{nullptr, hints.lazy_history}; // what this call's inner solve is told: the norm and the deferral only where they hold below
        if (use_preconditioner)
        {
            fdd_timer().start("subdomain.solver");
            if (composite_precond)
            {
                // full domain decomposition: the inner solve starts from the residual on the points (degree tree,
                // ring pull, coarse all-gather: Subdomain::tree_operator) and returns the composite's dof vector,
                // whose leading entries are this rank's nodes
                // (the own points' part of the right-hand side is the node residual itself when the dofs are a slice of the nodes)
                subdomain.gmres_composite_dofs(sub_u, rp, true, false, (dof_shift >= 0 and composite_rhs_from_nodes) ? rn.as<double>() + dof_shift : nullptr, inner);
            }
            else if (dof_shift >= 0)
            {
                // the dofs are the node slice [dof_shift, dof_shift + dofs): the inner solve reads r^ in place -- and, where
                // every stitching weight of the slice is exactly 1 (one rank: multiplicity * 1/multiplicity), writes z~ in
                // place as well: the multiplication below would be x * 1.0
                fdd::memory f_slice = rn.slice(dof_shift, nodes_sub_dofs);
                // the norm of this very slice was formed a moment ago (node_norm_enqueue): the inner solve starts from it
                inner.known_rhs_norm2 = hints.known_rhs_norm2;
                if (stitch_is_one and unit_stitch_in_place)
                {
                    fdd::memory z_slice = zn.slice(dof_shift, nodes_sub_dofs);
                    // nothing stands between the in-place update and the caller's pass: one rank, no exchange below
                    if (fdd::comm().size == 1) inner.defer_into = hints.defer_into;
                    subdomain.gmres_dofs(z_slice, f_slice, true, false, inner);
                }
                else
                    subdomain.gmres_dofs(sub_u, f_slice, true, false, inner);
            }
            else
            {
                FDD_CALL(fdd_gather_indexed(sub_f.as<double>(), rn.as<double>(), node_of_dof.as<int>(), nullptr, nodes_sub_dofs, stream));
                subdomain.gmres_dofs(sub_u, sub_f, true, false, inner);
            }
            fdd_timer().stop("subdomain.solver");

            fdd_timer().start("subdomain.stitching");
            if (dof_shift >= 0 and not composite_precond and stitch_is_one and unit_stitch_in_place)
            {
                // z~ is already in place
            }
            else if (dof_shift >= 0)
            {
                // the Dirichlet ends of z~ were cleared once (fcg_nodes_begin) and nothing writes them: the shared ones
                // see only zeros in the exchange (every rank masks them)
                FDD_CALL(fdd_amg_vector_multiplication(zn.as<double>() + dof_shift, sub_u.as<double>(), node_stitch.as<double>() + dof_shift, nodes_sub_dofs, stream));
            }
            else
                FDD_CALL(fdd_gather_indexed(zn.as<double>(), sub_u.as<double>(), dof_of_node.as<int>(), node_stitch.as<double>(), num_local_nodes, stream));
            if (norm_state.deferred)
            {
                gs_add_boundary_pair(zn, nprefix);
                node_norm_finish();
            }
            else
                gs_add_boundary(zn);
            fdd_timer().stop("subdomain.stitching");
        }
        else
        {
            nt.copyFrom(rn, (size_t)num_local_nodes * sizeof(DType));
            if (norm_state.deferred)
            {
                gs_add_boundary_pair(nt, nprefix);
                node_norm_finish();
            }
            else
                gs_add_boundary(nt);
            FDD_CALL(fdd_amg_vector_multiplication(zn.as<double>(), nt.as<double>(), node_mask.as<double>(), num_local_nodes, stream));
        }
    }

    template <typename PType>
    void fcg_nodes_begin(fdd::memory &u, fdd::memory &f, PType &subdomain)
    {
        setup_nodes();
        if (use_preconditioner) setup_dof_maps(subdomain);
        fcg.u_pts = u;
        fcg.nodes_active = true;

        gather_nodes(nr, f);
        if (use_preconditioner and composite_precond) rp.copyFrom(f, (size_t)num_local_points * sizeof(DType)); // r = f on the points as well
        FDD_CALL(fdd_set_to_value(nu.as<double>(), 0.0, num_local_nodes, 0, fdd::dev().stream));
        FDD_CALL(fdd_set_to_value(nz.as<double>(), 0.0, num_local_nodes, 0, fdd::dev().stream));

        const double *r0_norm2 = node_norm(fcg.r_0_norm, nr);
        residual_history.push_back(fcg.r_0_norm);
        rstdout("Iter %2d: | residual_norm = %24.16g | relative_residual_norm = %24.16g | \n", 0, fcg.r_0_norm, 1.0);

        precondition_nodes(nz, nr, subdomain, {r0_norm2});
        np.copyFrom(nz, (size_t)num_local_nodes * sizeof(DType));
        // (fcg.gamma_on_device is clear: the first iteration's projection kernel forms gamma itself)
    }

    DType fcg_nodes_step_residual()
    {
        const int nn = num_local_nodes;
        void *stream = fdd::dev().stream;
        DType values[2], r_norm;

        fcg_flush_solution_update(); // a residual half that follows another: alpha's operands are about to be overwritten

        fdd_timer().start("domain.operator_application");
        stiffness_from_nodes(q_k, np);
        gather_nodes(nq, q_k);
        fdd_timer().stop("domain.operator_application");

        if (device_scalars and fcg.gamma_on_device and early_gamma)
        {
            // gamma = <z, r> already sits in scalars[fcg.gamma_slot]: the flexible dot of the previous iteration formed it from the
            // vectors it was reading anyway (fcg_nodes_step_direction); <p, q> is what is left of domain.okl:140-184
            // (with a Helmholtz shift the same pass first completes q^ += c .* p~ and sums the values it stores)
            if (shift_active())
                FDD_CALL(fdd_shift_add_inner_product(scalars.as<double>() + SLOT_PQ, reduce_ws.as<double>(), nq.as<double>(), shift_nodes.as<double>(), np.as<double>(), nn, stream));
            else
                FDD_CALL(fdd_sub_inner_product(scalars.as<double>() + SLOT_PQ, reduce_ws.as<double>(), np.as<double>(), nq.as<double>(), nn, stream));
            if (fdd::comm().size > 1) fdd::comm().allreduce_sum(scalars.as<double>() + SLOT_PQ, 1);
        }
        else
        {
            shift_add_nodes(nq, np);
            FDD_CALL(fdd_dom_projection_inner_products(scalars.as<double>(), reduce_ws.as<double>(), nz.as<double>(), nr.as<double>(), np.as<double>(), nq.as<double>(), nn, stream));
            if (device_scalars and fdd::comm().size > 1) fdd::comm().allreduce_sum(scalars.as<double>(), 2);
        }
        if (device_scalars)
        {
            // gamma = scalars[fcg.gamma_slot] (kept for beta), theta = scalars[SLOT_PQ]: alpha never visits the host
            if (not(fcg.gamma_on_device and early_gamma)) fcg.gamma_slot = 0; // the projection kernel has just written it
            const double *a_num = scalars.as<double>() + fcg.gamma_slot, *a_den = scalars.as<double>() + SLOT_PQ;
            // u~ += alpha p~ is left to the direction half, which reads p~ anyway (nothing reads u~ before the solve ends)
            const bool defer_u = solution_in_direction_pass and &fdd_dom_solution_direction_update_dev != nullptr;
            // the norm of r+ over the dof slice is summed where r+ is stored
            const bool fuse_norm = fused_residual_norm and &fdd_dom_residual_update_norm2_dev != nullptr and norm_is_slice_sum();
            if (not defer_u and not fuse_norm)
                FDD_CALL(fdd_dom_solution_and_residual_update_dev(nu.as<double>(), nr1.as<double>(), nr.as<double>(), np.as<double>(), nq.as<double>(), a_num, a_den, nn, stream));
            else
            {
                // the two statements of that kernel, each where it costs least
                if (defer_u)
                    fcg.owed_u = {true, a_num, a_den};
                else
                    FDD_CALL(fdd_xpby_ratio_dev(nu.as<double>(), nu.as<double>(), a_num, a_den, np.as<double>(), nn, stream));
                if (fuse_norm)
                    fcg.pending_rhs_norm2 = residual_update_and_norm_enqueue(nr1, nr, nq, a_num, a_den);
                else
                    FDD_CALL(fdd_xmay_ratio_dev(nr1.as<double>(), nr.as<double>(), a_num, a_den, nq.as<double>(), nn, stream));
            }
            if (use_preconditioner and composite_precond) // r+ = r - alpha q on the points too (domain.okl:191), alpha from device memory
                FDD_CALL(fdd_xmay_ratio_dev(rp.as<double>(), rp.as<double>(), a_num, a_den, q_k.as<double>(), num_local_points, stream));
            if (not fuse_norm) fcg.pending_rhs_norm2 = node_norm_enqueue(nr1, /*defer_exchange=*/true); // finished inside the preconditioner's exchange
            fcg.norm_pending = true;
            return std::numeric_limits<DType>::quiet_NaN(); // fcg_nodes_norm() has the value
        }
        fetch_scalars(values, 2);
        fcg.gamma_k = values[0];
        const DType alpha_k = fcg.gamma_k / values[1];

        FDD_CALL(fdd_dom_solution_and_residual_update(nu.as<double>(), nr1.as<double>(), nr.as<double>(), np.as<double>(), nq.as<double>(), alpha_k, nn, stream));
        if (use_preconditioner and composite_precond) FDD_CALL(fdd_vector_vector_addition(rp.as<double>(), 1.0, rp.as<double>(), -alpha_k, q_k.as<double>(), num_local_points, stream));

        fcg.pending_rhs_norm2 = node_norm(r_norm, nr1);
        residual_history.push_back(r_norm);
        rstdout("Iter %2d: | residual_norm = %24.16g | relative_residual_norm = %24.16g | \n", fcg.iter + 1, r_norm, r_norm / fcg.r_0_norm);
        return r_norm;
    }

    // the residual norm enqueued by the last fcg_nodes_step_residual (device_scalars mode)
    DType fcg_nodes_norm()
    {
        const DType r_norm = node_norm_fetch();
        fcg.norm_pending = false;
        residual_history.push_back(r_norm);
        rstdout("Iter %2d: | residual_norm = %24.16g | relative_residual_norm = %24.16g | \n", fcg.iter + 1, r_norm, r_norm / fcg.r_0_norm);
        return r_norm;
    }

    template <typename PType>
    void fcg_nodes_step_direction(PType &subdomain, bool lazy_history = false)
    {
        const int nn = num_local_nodes;
        DType theta_k;
        // the inner solve's final update of z~ may ride in the flexible dot's pass below, which reads z~ first
        const bool fuse_update = fused_update_flexible_dot and device_scalars and early_gamma and &fdd_dom_lincomb_flexible_gamma != nullptr;
        fdd::PendingUpdate pu; // owed from the inner solve's return to the flexible dot below
        // nr1 is untouched since its norm was enqueued (fcg_nodes_step_residual)
        precondition_nodes(nz, nr1, subdomain, {fcg.pending_rhs_norm2, lazy_history, fuse_update ? &pu : nullptr});
        fcg.pending_rhs_norm2 = nullptr;
        if (device_scalars)
        {
            // beta = theta / gamma, read by the update kernel; the residual norm's two parts sit right behind theta
            // (SLOT_THETA, SLOT_NORM) and are summed over the ranks in the same collective
            int theta_at = SLOT_THETA;
            if (early_gamma)
            {
                // {<z, r+> (the next iteration's gamma), theta} from one pass over r, r+, z.  The pair alternates between
                // SLOT_PAIR_A and SLOT_PAIR_B (the current gamma must outlive it: beta reads it below), either side of
                // the norm's two parts, so that one all-reduce still carries all four
                const int next = (fcg.gamma_slot == SLOT_PAIR_A) ? SLOT_PAIR_B : SLOT_PAIR_A;
                theta_at = next + 1;
                if (pu.active)
                {
                    // z~'s dof slice is formed here, by the statement the inner solve would have launched, and enters the two
                    // sums without a trip through memory; the inner right-hand side (r+'s slice) is read once for both
                    pu.active = false;
                    if (pu.q != nz.as<double>() + dof_shift or pu.n > nodes_sub_dofs)
                    {
                        fprintf(stderr, "ERROR: the inner solve's deferred update is not the one of z~'s dof slice\n");
                        exit(EXIT_FAILURE);
                    }
                    const bool rhs_shared = pu.v[0] == nr1.as<double>() + dof_shift;
                    fdd::ProfileScope prof("reduce_vec2_kernel<LincombFlexGamma>", 8.0 * (2.0 * nn + (nn - pu.n) + (double)pu.n * ((double)pu.v.size() + (rhs_shared ? 0 : 1))));
                    FDD_CALL(fdd_dom_lincomb_flexible_gamma(scalars.as<double>() + next, reduce_ws.as<double>(), nr.as<double>(), nr1.as<double>(), nz.as<double>(), nn, dof_shift, pu.n, pu.q_is_zero, pu.coeffs_dev, pu.v.data(),
                                                            pu.scales_dev, pu.last_dev, (int)pu.v.size(), fdd::dev().stream));
                }
                else
                    FDD_CALL(fdd_dom_inner_product_flexible_gamma(scalars.as<double>() + next, reduce_ws.as<double>(), nr.as<double>(), nr1.as<double>(), nz.as<double>(), nn, fdd::dev().stream));
                if (fdd::comm().size > 1)
                {
                    if (norm_state.reduce_pending)
                        fdd::comm().allreduce_sum(scalars.as<double>() + std::min(next, SLOT_NORM), 4); // pair A + norm, or norm + pair B
                    else
                        fdd::comm().allreduce_sum(scalars.as<double>() + next, 2);
                }
                norm_state.reduce_pending = false;
                // p = z + beta p; "r = r+" (domain.okl:226-233) is a swap of the two node vectors, not a copy
                direction_update_dev(scalars.as<double>() + theta_at, scalars.as<double>() + fcg.gamma_slot);
                fcg.gamma_slot = next;
            }
            else
            {
                FDD_CALL(fdd_dom_inner_product_flexible(scalars.as<double>() + SLOT_THETA, reduce_ws.as<double>(), nr.as<double>(), nr1.as<double>(), nz.as<double>(), nn, fdd::dev().stream));
                if (fdd::comm().size > 1) fdd::comm().allreduce_sum(scalars.as<double>() + SLOT_THETA, norm_state.reduce_pending ? 3 : 1);
                norm_state.reduce_pending = false;
                direction_update_dev(scalars.as<double>() + SLOT_THETA, scalars.as<double>() + fcg.gamma_slot);
            }
            fcg.gamma_on_device = early_gamma;
            std::swap(nr, nr1);
        }
        else
        {
            fcg.gamma_on_device = false;
            fcg_flush_solution_update(); // (device_scalars was cleared between the halves: p~ changes below)
            FDD_CALL(fdd_dom_inner_product_flexible(scalars.as<double>(), reduce_ws.as<double>(), nr.as<double>(), nr1.as<double>(), nz.as<double>(), nn, fdd::dev().stream));
            fetch_scalars(&theta_k, 1);
            const DType beta_k = theta_k / fcg.gamma_k;
            FDD_CALL(fdd_dom_residual_and_search_update(np.as<double>(), nr.as<double>(), nz.as<double>(), nr1.as<double>(), beta_k, nn, fdd::dev().stream));
        }
        if (pu.active)
        {
            // the inner solve left its final update to this function and no branch above formed it: z~ was never written
            fprintf(stderr, "ERROR: an inner solve's deferred final update was dropped\n");
            exit(EXIT_FAILURE);
        }
        num_iterations++;
        fcg.iter++;
    }

    // p~ = z~ + beta p~, beta = *b_num / *b_den, and with it the solution update the residual half left owed
    void direction_update_dev(const double *b_num, const double *b_den)
    {
        const int nn = num_local_nodes;
        if (fcg.owed_u.active)
        {
            // alpha's operands (the current gamma and <p, q>) are still in their slots: gamma_slot only advances behind this pass
            fdd::ProfileScope prof("ew_kernel<SolutionDirectionDev>", 40.0 * nn);
            FDD_CALL(fdd_dom_solution_direction_update_dev(nu.as<double>(), np.as<double>(), nz.as<double>(), fcg.owed_u.num, fcg.owed_u.den, b_num, b_den, nn, fdd::dev().stream));
            fcg.owed_u.active = false;
        }
        else
            FDD_CALL(fdd_xpby_ratio_dev(np.as<double>(), nz.as<double>(), b_num, b_den, np.as<double>(), nn, fdd::dev().stream));
    }

    // the owed solution update as a launch of its own (the statement of the kernel it was taken out of): in front of whatever
    // reads u~, or overwrites p~ or alpha's operands, while it is owed
    void fcg_flush_solution_update()
    {
        if (not fcg.owed_u.active) return;
        FDD_CALL(fdd_xpby_ratio_dev(nu.as<double>(), nu.as<double>(), fcg.owed_u.num, fcg.owed_u.den, np.as<double>(), num_local_nodes, fdd::dev().stream));
        fcg.owed_u.active = false;
    }

    // u = Q u~: hand the solution back on the element-local points
    void fcg_finish()
    {
        if (not fcg.nodes_active) return;
        fcg_flush_solution_update();
        Q.multiply(fcg.u_pts, nu);
    }

    // domain.tpp:611-725.  The loop body is exposed as fcg_begin / fcg_step so
    // that a caller (bench.py) can time an exact number of iterations; the
    // method itself is begin + steps + the reference's stopping tests.
    template <typename PType>
    void fcg_begin(fdd::memory &u, fdd::memory &f, PType &subdomain)
    {
        residual_history.clear();
        num_iterations = 0;
        fcg = FcgRun();
        norm_state = NormInFlight();
        if (can_fcg_nodes(subdomain))
        {
            fcg_nodes_begin(u, f, subdomain);
            return;
        }
        fcg.u = u;

        fdd_timer().start("domain.vector_operations");
        FDD_CALL(fdd_dom_initialize_arrays(u.as<double>(), r_k.as<double>(), f.as<double>(), num_local_points, fdd::dev().stream));
        fdd_timer().stop("domain.vector_operations");

        fdd_timer().start("domain.residual_norm");
        residual_norm(fcg.r_0_norm, r_k);
        fdd_timer().stop("domain.residual_norm");

        residual_history.push_back(fcg.r_0_norm);
        rstdout("Iter %2d: | residual_norm = %24.16g | relative_residual_norm = %24.16g | \n", 0, fcg.r_0_norm, 1.0);

        apply_preconditioner(z_k, r_k, subdomain);

        fdd_timer().start("domain.vector_operations");
        p_k.copyFrom(z_k, (size_t)num_local_points * sizeof(DType));
        fdd_timer().stop("domain.vector_operations");
    }

    // first half of an iteration: q = A p, alpha, u += alpha p, r+ = r - alpha q, ||r+||
    DType fcg_step_residual()
    {
        if (fcg.nodes_active) return fcg_nodes_step_residual();
        DType theta_k, r_norm;

        fdd_timer().start("domain.operator_application");
        stiffness_matrix(q_k, p_k);
        fdd_timer().stop("domain.operator_application");

        fdd_timer().start("domain.inner_products");
        projection_inner_products(fcg.gamma_k, theta_k, z_k, r_k, p_k, q_k);
        fdd_timer().stop("domain.inner_products");

        const DType alpha_k = fcg.gamma_k / theta_k;

        fdd_timer().start("domain.vector_operations");
        solution_and_residual_update(fcg.u, r_kp1, r_k, p_k, q_k, alpha_k);
        fdd_timer().stop("domain.vector_operations");

        fdd_timer().start("domain.residual_norm");
        residual_norm(r_norm, r_kp1);
        fdd_timer().stop("domain.residual_norm");

        residual_history.push_back(r_norm);
        rstdout("Iter %2d: | residual_norm = %24.16g | relative_residual_norm = %24.16g | \n", fcg.iter + 1, r_norm, r_norm / fcg.r_0_norm);
        return r_norm;
    }

    // second half: z = M^-1 r+ (+ stitching), beta, p = z + beta p, r = r+
    template <typename PType>
    void fcg_step_direction(PType &subdomain)
    {
        if (fcg.nodes_active)
        {
            fcg_nodes_step_direction(subdomain);
            return;
        }
        DType theta_k;

        apply_preconditioner(z_k, r_kp1, subdomain);

        fdd_timer().start("domain.inner_products");
        inner_product_flexible(theta_k, r_k, r_kp1, z_k);
        fdd_timer().stop("domain.inner_products");

        const DType beta_k = theta_k / fcg.gamma_k;

        fdd_timer().start("domain.vector_operations");
        residual_and_search_update(p_k, r_k, z_k, r_kp1, beta_k);
        fdd_timer().stop("domain.vector_operations");

        num_iterations++;
        fcg.iter++;
    }

    // one full PCG iteration without stopping tests (what bench.py calls a step)
    template <typename PType>
    DType fcg_step(PType &subdomain)
    {
        DType r_norm = fcg_step_residual();
        if (fcg.norm_pending)
        {
            // the norm's reductions are in the queue; the preconditioner is enqueued behind them
            // before the host waits for the value (the inner solve synchronises at its end anyway)
            fcg_step_direction(subdomain);
            fcg.iter--; // the history line belongs to the iteration just counted
            r_norm = fcg_nodes_norm();
            fcg.iter++;
            return r_norm;
        }
        fcg_step_direction(subdomain);
        return r_norm;
    }

    // K iterations without stopping tests (what bench.py times).  In the node-space / device-scalar mode nothing
    // in an iteration needs the host: the norms go to a device-side history and are read once at the end, the
    // inner solves run without their end-of-cycle read (InnerSolveHints::lazy_history).  Same arithmetic, same order.
    template <typename PType>
    DType fcg_steps(PType &subdomain, int K)
    {
        DType r_norm = std::numeric_limits<DType>::quiet_NaN();
        if (K <= 0) return r_norm;
        if (not(fcg.nodes_active and device_scalars and lazy_steps))
        {
            for (int s = 0; s < K; s++) r_norm = fcg_step(subdomain);
            return r_norm;
        }
        if (norm_hist_cap < K)
        {
            norm_hist = fdd::dev().malloc<DType>(K);
            norm_hist_cap = K;
        }
        for (int s = 0; s < K; s++)
        {
            fcg_nodes_step_residual();
            fcg_nodes_step_direction(subdomain, /*lazy_history=*/true);
            FDD_CALL(fdd_sqrt_sum_dev(norm_hist.as<double>() + s, scalars.as<double>() + SLOT_NORM, norm_state.parts, fdd::dev().stream));
            fcg.norm_pending = false;
        }
        std::vector<DType> h(K);
        norm_hist.copyTo(h.data(), (size_t)K * sizeof(DType)); // the one synchronisation of the K iterations
        for (int s = 0; s < K; s++)
        {
            residual_history.push_back(h[s]);
            rstdout("Iter %2d: | residual_norm = %24.16g | relative_residual_norm = %24.16g | \n", fcg.iter - K + s + 1, h[s], h[s] / fcg.r_0_norm);
        }
        return h[K - 1];
    }

    template <typename PType>
    void flexible_conjugate_gradient(fdd::memory &u, fdd::memory &f, PType &subdomain, bool use_relative = true)
    {
        fcg_begin(u, f, subdomain);

        for (int iter = 0; iter < max_iterations; iter++)
        {
            DType r_norm = fcg_step_residual();
            bool direction_done = false;
            if (fcg.norm_pending)
            {
                // device_scalars: the second half of the iteration is enqueued before the host reads
                // the norm.  If the tests below stop the solve, that half was speculative: it touched
                // z, p, r and, of the solution, only the update it owed to the iteration whose residual
                // has just been tested (solution_in_direction_pass) -- the solution returned is that
                // iteration's either way -- and its iteration count is taken back.
                fcg_step_direction(subdomain);
                direction_done = true;
                fcg.iter--;
                r_norm = fcg_nodes_norm();
                fcg.iter++;
            }

            bool stop = use_relative ? (r_norm / fcg.r_0_norm < tolerance) : (r_norm < tolerance);
            if (std::isnan(r_norm)) stop = true;
            if (stop)
            {
                if (direction_done)
                {
                    num_iterations--;
                    fcg.iter--;
                }
                break;
            }

            if (not direction_done) fcg_step_direction(subdomain);
        }
        fcg_finish();
    }

    // ------------------------------------------------------------------
    // Node-space flexible GMRES(m): the recurrences of domain.tpp:727-914 on one value per assembled node.  The outer
    // iteration sees its dual vectors (r, q, V_i) only through Qt -- <a, b> = sum_points a (QQt b) mask = sum_nodes
    // (Qt a) gs(Qt b) mask -- and its continuous ones (Z_j, u) only through Q, so basis, preconditioned basis, residual
    // and solution are node vectors (0.68 x the points at N = 7), an operator application is the gather-on-load stiffness
    // + one Qt gather, and no direct-stiffness summation is left: with more than one rank the interface prefix of a new
    // basis vector is exchanged once (VNA) and the norm exchanges its own.  Same Hessenberg entries, rotations, stopping
    // tests and iteration count as the point-space form to rounding (test_reference_shaped_and_restructured_paths_agree).
    // On a composite the basis is kept on the points as well: the preconditioner's degree tree restricts point data.
    // ------------------------------------------------------------------
    template <typename PType>
    void gmres_nodes(fdd::memory &u, fdd::memory &f, PType &subdomain, bool use_relative)
    {
        setup_nodes();
        if (use_preconditioner) setup_dof_maps(subdomain);
        const int nn = num_local_nodes, m = num_vectors;
        void *stream = fdd::dev().stream;
        const bool multi = fdd::comm().size > 1 and num_interface_slots > 0; // rank-uniform
        const bool points_too = use_preconditioner and composite_precond;
        if (gmres_nodes_vectors != m or (multi and VNA.empty()) or (points_too and VP.empty()))
        {
            for (auto *set : {&VN, &ZN, &VNA, &VP}) set->clear();
            nf = fdd::dev().malloc<DType>(std::max(nn, 1));
            VN.resize(m + 1);
            for (auto &v : VN) v = fdd::dev().malloc<DType>(std::max(nn, 1));
            ZN.resize(m);
            for (auto &v : ZN)
            {
                v = fdd::dev().malloc<DType>(std::max(nn, 1));
                FDD_CALL(fdd_set_to_value(v.as<double>(), 0.0, nn, 0, stream)); // the Dirichlet ends stay zero: nothing writes them
            }
            if (multi)
            {
                VNA.resize(m + 1);
                for (auto &v : VNA) v = fdd::dev().malloc<DType>(std::max(nn, 1));
            }
            if (points_too)
            {
                VP.resize(m + 1);
                for (auto &v : VP) v = fdd::dev().malloc<DType>(std::max(num_local_points, 1));
            }
            gmres_nodes_vectors = m;
        }
        residual_history.clear();
        norm_state = NormInFlight();

        // the assembled copy <., .> reads: gs over the ranks on the interface prefix, nothing to do on one rank
        auto assembled = [&](int i) -> fdd::memory & {
            if (not multi) return VN[i];
            VNA[i].copyFrom(VN[i], (size_t)nn * sizeof(DType));
            gs_add_boundary(VNA[i]);
            return VNA[i];
        };
        auto norm_of = [&](fdd::memory &v) {
            DType norm;
            fdd_timer().start("domain.residual_norm");
            node_norm(norm, v);
            fdd_timer().stop("domain.residual_norm");
            return norm;
        };

        fdd_timer().start("domain.vector_operations");
        gather_nodes(nf, f); // f^ = Qt f
        fcg.owed_u.active = false; // u~ is this solve's from here on
        FDD_CALL(fdd_set_to_value(nu.as<double>(), 0.0, nn, 0, stream));
        nr.copyFrom(nf, (size_t)nn * sizeof(DType));
        if (points_too) VP[0].copyFrom(f, (size_t)num_local_points * sizeof(DType));
        fdd_timer().stop("domain.vector_operations");

        std::vector<const double *> va(m + 1, nullptr); // assembled basis of the current cycle
        std::vector<DType> minus_h(m);
        fdd::GmresSpace<DType> space;
        space.initial_norm = [&] { return norm_of(nr); };
        space.restart_norm = [&] {
            fdd_timer().start("domain.operator_application");
            stiffness_from_nodes(q_k, nu);
            gather_nodes(nq, q_k);
            shift_add_nodes(nq, nu);
            fdd_timer().stop("domain.operator_application");
            fdd_timer().start("domain.vector_operations");
            FDD_CALL(fdd_vector_vector_addition(nr.as<double>(), 1.0, nf.as<double>(), -1.0, nq.as<double>(), nn, stream));
            if (points_too) FDD_CALL(fdd_vector_vector_addition(VP[0].as<double>(), 1.0, f.as<double>(), -1.0, q_k.as<double>(), num_local_points, stream));
            fdd_timer().stop("domain.vector_operations");
            return norm_of(nr);
        };
        space.start_cycle = [&](DType gamma_0) {
            fdd_timer().start("domain.vector_operations");
            FDD_CALL(fdd_vector_scaling(VN[0].as<double>(), 1.0 / gamma_0, nr.as<double>(), nn, stream));
            if (points_too) FDD_CALL(fdd_vector_scaling(VP[0].as<double>(), 1.0 / gamma_0, VP[0].as<double>(), num_local_points, stream));
            fdd_timer().stop("domain.vector_operations");
            va[0] = assembled(0).template as<double>();
        };
        space.arnoldi_step = [&](int j, std::vector<std::vector<DType>> &H) {
            if (points_too) rp.copyFrom(VP[j], (size_t)num_local_points * sizeof(DType)); // the tree restricts V_j on the points
            precondition_nodes(ZN[j], VN[j], subdomain);

            fdd_timer().start("domain.operator_application");
            stiffness_from_nodes(q_k, ZN[j]);
            gather_nodes(nq, q_k);
            shift_add_nodes(nq, ZN[j]);
            fdd_timer().stop("domain.operator_application");

            // classical Gram-Schmidt: every H[i][j] from the same q (domain.tpp:810-815), then the updates
            fdd_timer().start("domain.inner_products");
            grouped_inner_products(H, j, nq, va.data(), j + 1, node_mask, nn);
            fdd_timer().stop("domain.inner_products");

            fdd_timer().start("domain.vector_operations");
            for (int i = 0; i < j + 1; i++) minus_h[i] = -H[i][j];
            grouped_axpy(nq, minus_h.data(), VN, j + 1, nn);
            if (points_too) grouped_axpy(q_k, minus_h.data(), VP, j + 1, num_local_points);
            fdd_timer().stop("domain.vector_operations");
            return norm_of(nq);
        };
        space.next_vector = [&](int j, DType alpha_j) {
            fdd_timer().start("domain.vector_operations");
            FDD_CALL(fdd_vector_scaling(VN[j + 1].as<double>(), 1.0 / alpha_j, nq.as<double>(), nn, stream));
            if (points_too) FDD_CALL(fdd_vector_scaling(VP[j + 1].as<double>(), 1.0 / alpha_j, q_k.as<double>(), num_local_points, stream));
            fdd_timer().stop("domain.vector_operations");
            if (j + 1 < m) va[j + 1] = assembled(j + 1).template as<double>(); // the last vector of a cycle is never projected on
        };
        space.add_update = [&](int j, const std::vector<DType> &c) {
            fdd_timer().start("domain.vector_operations");
            grouped_axpy(nu, c.data(), ZN, j + 1, nn);
            fdd_timer().stop("domain.vector_operations");
        };
        num_iterations = fdd::gmres_solve(gmres_scalars, m, outer_gmres_control(use_relative), space, residual_history, print_outer_step);

        Q.multiply(u, nu); // the solution back on the element-local points
    }

    // domain.tpp:727-914
    template <typename PType>
    void generalized_minimum_residual(fdd::memory &u, fdd::memory &f, PType &subdomain, bool use_relative = true)
    {
        if (restructured_outer and can_fcg_nodes(subdomain))
        {
            gmres_nodes(u, f, subdomain, use_relative);
            return;
        }
        allocate_gmres();
        residual_history.clear();

        fdd_timer().start("domain.vector_operations");
        fdd::memory &u_k = u;
        FDD_CALL(fdd_dom_initialize_arrays(u_k.as<double>(), r_k.as<double>(), f.as<double>(), num_local_points, fdd::dev().stream));
        fdd_timer().stop("domain.vector_operations");

        auto norm_of = [&](fdd::memory &v) {
            DType norm;
            fdd_timer().start("domain.residual_norm");
            residual_norm(norm, v);
            fdd_timer().stop("domain.residual_norm");
            return norm;
        };
        std::vector<const double *> va(num_vectors);
        std::vector<DType> minus_h(num_vectors);
        fdd::GmresSpace<DType> space;
        space.initial_norm = [&] { return norm_of(r_k); };
        space.restart_norm = [&] {
            fdd_timer().start("domain.operator_application");
            stiffness_matrix(r_k, u_k);
            fdd_timer().stop("domain.operator_application");

            fdd_timer().start("domain.vector_operations");
            math.vector_vector_addition(r_k, 1.0, f, -1.0, r_k, num_local_points);
            fdd_timer().stop("domain.vector_operations");
            return norm_of(r_k);
        };
        space.start_cycle = [&](DType gamma_0) {
            fdd_timer().start("domain.vector_operations");
            math.vector_scaling(V[0], 1.0 / gamma_0, r_k, num_local_points);
            fdd_timer().stop("domain.vector_operations");
            va_valid = 0; // a new basis
        };
        space.arnoldi_step = [&](int j, std::vector<std::vector<DType>> &H) {
            apply_preconditioner(Z[j], V[j], subdomain);

            fdd_timer().start("domain.operator_application");
            stiffness_matrix(q_k, Z[j]);
            fdd_timer().stop("domain.operator_application");

            // classical Gram-Schmidt: every H[i][j] from the same q_k (domain.tpp:810-815)
            if (restructured_outer)
            {
                // <q, V_i> = sum q * (QQt V_i) * mask with the assembled copy VA[i] = mask * QQt V_i cached when
                // V_i was made (the reference redoes the dssum inside each of the (j+1)(j+2)/2 products);
                // the (j+1) dots read q once per group of FDD_MULTI_MAX, the (j+1) updates are one pass per group
                fdd_timer().start("domain.inner_products");
                gmres_cache_assembled(j);
                for (int i = 0; i < j + 1; i++) va[i] = VA[i].template as<double>();
                grouped_inner_products(H, j, q_k, va.data(), j + 1, dirichlet_mask, num_local_points);
                fdd_timer().stop("domain.inner_products");

                fdd_timer().start("domain.vector_operations");
                for (int i = 0; i < j + 1; i++) minus_h[i] = -H[i][j];
                grouped_axpy(q_k, minus_h.data(), V, j + 1, num_local_points);
                fdd_timer().stop("domain.vector_operations");
            }
            else
            {
                for (int i = 0; i < j + 1; i++)
                {
                    fdd_timer().start("domain.inner_products");
                    assembled_inner_product(H[i][j], q_k, V[i]);
                    fdd_timer().stop("domain.inner_products");
                }

                for (int i = 0; i < j + 1; i++)
                {
                    fdd_timer().start("domain.vector_operations");
                    math.vector_vector_addition(q_k, 1.0, q_k, -H[i][j], V[i], num_local_points);
                    fdd_timer().stop("domain.vector_operations");
                }
            }
            return norm_of(q_k);
        };
        space.next_vector = [&](int j, DType alpha_j) {
            fdd_timer().start("domain.vector_operations");
            math.vector_scaling(V[j + 1], 1.0 / alpha_j, q_k, num_local_points);
            fdd_timer().stop("domain.vector_operations");
        };
        space.add_update = [&](int j, const std::vector<DType> &c) {
            if (restructured_outer)
            {
                fdd_timer().start("domain.vector_operations");
                grouped_axpy(u_k, c.data(), Z, j + 1, num_local_points);
                fdd_timer().stop("domain.vector_operations");
                return;
            }
            for (int i = 0; i < j + 1; i++)
            {
                fdd_timer().start("domain.vector_operations");
                math.vector_vector_addition(u_k, 1.0, u_k, c[i], Z[i], num_local_points);
                fdd_timer().stop("domain.vector_operations");
            }
        };
        num_iterations = fdd::gmres_solve(gmres_scalars, num_vectors, outer_gmres_control(use_relative), space, residual_history, print_outer_step);
    }

    // ------------------------------------------------------------------
    // Successive-right-hand-side projection (projection.hpp; an addition of this build).  Off (capacity 0) unless
    // configured; the solvers above are called unchanged.
    // ------------------------------------------------------------------
    fdd::Projection projection;

    // The outer solve (solver_id 0: flexible CG, 1: GMRES) of A u = f started from x0 = X (X^T f), the best approximation
    // in the A-norm the basis holds; f is overwritten by f' = f - AX (X^T f).  It stops where the plain solve stops,
    // |r| <= tolerance |f| -- the solvers take that as an absolute tolerance for the duration of the call, and a start
    // value that already meets it costs no iteration (they always take a step before they test).  The correction delta
    // is then A-orthogonalised against the basis in one classical Gram-Schmidt sweep and stored with its image; a full
    // basis restarts from the solution alone, as Nek5000 does.  proj = {|f|, |f'|, rows used, rows afterwards}.
    // Dots are plain sums over the local points (the basis is continuous and zero on Dirichlet points, f and the images
    // are unassembled), summed over the ranks; every rank takes the same branches because they hang on those sums.
    template <typename PType>
    void solve_projected(fdd::memory &u, fdd::memory &f, PType &subdomain, int solver_id, DType proj[4])
    {
        fdd::Projection &pj = projection;
        void *stream = fdd::dev().stream;
        const int n = num_local_points, K = pj.size;
        const bool multi = fdd::comm().size > 1;
        double *ws = reduce_ws.as<double>(), *c = pj.c.as<double>();
        auto solve = [&](fdd::memory &out, bool use_relative) {
            if (solver_id == 0)
                flexible_conjugate_gradient(out, f, subdomain, use_relative);
            else
                generalized_minimum_residual(out, f, subdomain, use_relative);
        };
        auto nothing_to_iterate = [&](DType r_norm) {
            residual_history.assign(1, r_norm);
            num_iterations = 0;
        };

        DType b_norm, r_norm;
        residual_norm(b_norm, f);
        proj[0] = proj[1] = b_norm;
        proj[2] = proj[3] = K;
        if (b_norm == 0.0)
        {
            FDD_CALL(fdd_set_to_value(u.as<double>(), 0.0, n, 0, stream));
            nothing_to_iterate(0.0);
            return;
        }
        if (pj.capacity == 0) // off: the plain solve, nothing stored
        {
            solve(u, true);
            return;
        }

        r_norm = b_norm;
        if (K > 0)
        {
            pj.dots(c, ws, f.as<double>());
            if (multi) fdd::comm().allreduce_sum(c, K);
            pj.apply(pj.x0.as<double>(), f.as<double>(), nullptr, ws, nullptr, f.as<double>(), c, 1.0, -1.0);
            residual_norm(r_norm, f);
            proj[1] = r_norm;
        }
        if (r_norm <= tolerance * b_norm)
        {
            if (K > 0)
                u.copyFrom(pj.x0, (size_t)n * sizeof(DType));
            else
                FDD_CALL(fdd_set_to_value(u.as<double>(), 0.0, n, 0, stream));
            nothing_to_iterate(r_norm);
            return;
        }

        // delta: into u itself while there is nothing to add it to
        fdd::memory &delta = (K > 0) ? pj.d : u;
        const DType relative_tolerance = tolerance;
        tolerance = relative_tolerance * b_norm;
        solve(delta, false);
        tolerance = relative_tolerance;
        if (K > 0) FDD_CALL(fdd_vector_vector_addition(u.as<double>(), 1.0, pj.x0.as<double>(), 1.0, delta.as<double>(), n, stream));

        // the basis update: w = A_L delta, e0 = <delta, w>, beta = X^T w, (delta, w) -= (X, AX) beta, nu2 = <delta, w>
        stiffness_matrix(pj.w, delta);
        double *e0_dev = c + K, *nu2_dev = c + K + 1;
        DType e0, nu2;
        FDD_CALL(fdd_sub_inner_product(e0_dev, ws, delta.as<double>(), pj.w.as<double>(), n, stream));
        if (K > 0)
        {
            pj.dots(c, ws, pj.w.as<double>());
            if (multi) fdd::comm().allreduce_sum(c, K + 1);
            pj.apply(delta.as<double>(), pj.w.as<double>(), nu2_dev, ws, delta.as<double>(), pj.w.as<double>(), c, -1.0, -1.0);
            if (multi) fdd::comm().allreduce_sum(nu2_dev, 1);
            DType both[2];
            pj.c.slice(K, 2).copyTo(both, sizeof(both));
            e0 = both[0];
            nu2 = both[1];
        }
        else
        {
            if (multi) fdd::comm().allreduce_sum(e0_dev, 1);
            pj.c.slice(K, 1).copyTo(&e0, sizeof(DType));
            nu2 = e0;
            nu2_dev = e0_dev;
        }
        // below 2^-52 e0 what is left of delta is the rounding of the sweep
        if (not std::isfinite(nu2) or not(nu2 > std::ldexp(e0, -52))) return;
        if (K == pj.capacity)
        {
            // full: start again from the solution alone, u / |u|_A (one more operator application)
            pj.restarts++;
            pj.size = 0;
            stiffness_matrix(pj.w, u);
            FDD_CALL(fdd_sub_inner_product(c, ws, u.as<double>(), pj.w.as<double>(), n, stream));
            if (multi) fdd::comm().allreduce_sum(c, 1);
            pj.c.copyTo(&nu2, sizeof(DType));
            if (std::isfinite(nu2) and nu2 > 0.0)
            {
                pj.store(0, u.as<double>(), pj.w.as<double>(), c);
                pj.size = 1;
            }
        }
        else
        {
            pj.store(K, delta.as<double>(), pj.w.as<double>(), nu2_dev);
            pj.size = K + 1;
        }
        proj[3] = pj.size;
    }
};

#endif
