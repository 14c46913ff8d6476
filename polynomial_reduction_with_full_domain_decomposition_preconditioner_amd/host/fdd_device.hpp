/*
 * fdd_device.hpp -- the thin layer that stands where OCCA stood.
 *
 * fdd::memory mirrors the slice of occa::memory the reference's host classes
 * use (copyFrom / copyTo / slice / ptr / free; usage inventory in SURVEY.md
 * section 8(b)) and fdd::device_t mirrors occa::device (malloc<T>, finish),
 * both over the C-ABI of include/fdd_hip.h.  Slices are pointer arithmetic on a shared block.
 * A failing C-ABI call prints and exits, the reference's own error style
 * (csr_matrix.tpp:72-76).
 */
#ifndef FDD_DEVICE_HPP
#define FDD_DEVICE_HPP

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "fdd_hip.h"

// The AMG setup entries (fdd_hip.h, "AMG setup on the device") are referenced weakly: a kernel library without them
// (an older libfdd_hip, a CPU stand-in of its C-ABI) still loads, and the switch that needs them ("amg_device_setup")
// refuses to turn on, naming the missing entry (missing_amg_setup_entry).
#pragma weak fdd_amg_setup_row_pointers
#pragma weak fdd_amg_setup_spgemm_count
#pragma weak fdd_amg_setup_spgemm_fill
#pragma weak fdd_amg_setup_transpose_count
#pragma weak fdd_amg_setup_transpose_fill
#pragma weak fdd_amg_setup_fem_stencils
#pragma weak fdd_amg_setup_fem_count
#pragma weak fdd_amg_setup_fem_fill
#pragma weak fdd_amg_setup_inv_sqrt_diagonal
#pragma weak fdd_amg_setup_unit_values
#pragma weak fdd_amg_setup_lattice_dofs
#pragma weak fdd_amg_setup_lattice_coarse_flags
#pragma weak fdd_amg_setup_lattice_cmap
#pragma weak fdd_amg_setup_lattice_interp_count
#pragma weak fdd_amg_setup_lattice_interp_fill
#pragma weak fdd_amg_setup_lattice_coarse_points
#pragma weak fdd_amg_setup_memory_info
// likewise the fused update-and-dot entry: without it the update and the dot stay two launches (Domain::fcg_nodes_step_direction)
#pragma weak fdd_dom_lincomb_flexible_gamma
// and the two passes of the outer step that carry a neighbour's work: without them the residual update, its norm, the solution
// update and the direction update stay the launches they were (Domain::fcg_nodes_step_residual / _direction)
#pragma weak fdd_dom_residual_update_norm2_dev
#pragma weak fdd_dom_solution_direction_update_dev
// and the projection passes: without them the same steps are composed from the multi-vector entries (projection.hpp), and the
// flag "fused_projection" refuses to be set to 1, naming the missing entry (missing_projection_entry)
#pragma weak fdd_projection_dots
#pragma weak fdd_projection_apply
#pragma weak fdd_projection_store
// and the steps of the Chebyshev-Jacobi inner solve: without them a step is composed from vector_vector_addition and
// vector_diagonal_scaling_dev (Subdomain::chebyshev_dofs, same bits), and the flags "chebyshev_kernels" / "fused_chebyshev"
// refuse to be set to 1, naming the missing entry (missing_chebyshev_entry)
#pragma weak fdd_cheby_step
#pragma weak fdd_cheby_step_f32
#pragma weak fdd_csr_plan_gather_cheby
#pragma weak fdd_csr_plan_gather_cheby_f32
// and the stiffness kernel that does not stream factor arrays that are identically zero, with its check: without them every
// list streams six arrays, and the flag "skip_zero_factors" refuses to be set to 1, naming the missing entry (here and below:
// set_stiffness_flag and the table of flags, element_operator.hpp)
#pragma weak fdd_stiffness_matrix_diag
#pragma weak fdd_stiffness_matrix_diag_f32
#pragma weak fdd_stiffness_offdiag_zero
// and its matrix-core instance (degree 11..15): without it those lists keep the six-array matrix-core kernel, and the flag
// "mfma_skip_zero_factors" refuses to be set to 1
#pragma weak fdd_stiffness_matrix_mfma_diag
// and the line form of the stiffness kernel at degree 7: without it those lists stay on the slab form, and the flag
// "line_stiffness" refuses to be set to 1, naming the missing entry
#pragma weak fdd_stiffness_matrix_lines
#pragma weak fdd_stiffness_matrix_lines_f32
// and its instance for factor blocks that repeat from element to element, with the two entries that establish which do:
// without them every list streams its own blocks, and the flag "shared_factor_blocks" refuses to be set to 1, naming the
// missing entry
#pragma weak fdd_stiffness_matrix_lines_shared
#pragma weak fdd_stiffness_matrix_lines_shared_f32
#pragma weak fdd_stiffness_factor_block_hash
#pragma weak fdd_stiffness_factor_block_verify
// and the lean instances of the line form (a D_hat with a zero interior diagonal that is its own negated mirror image):
// without them every list keeps the parent instance, and the flag "lean_line_stiffness" refuses to be set to 1, naming the
// missing entry
#pragma weak fdd_stiffness_matrix_lines_lean
#pragma weak fdd_stiffness_matrix_lines_lean_f32
// and the line form that completes most rows of the gather Qt itself, with the gather of the rows it leaves: without them
// every operator application keeps the point buffer and the whole gather, and the flag "assemble_in_stiffness" refuses to be
// set to 1, naming the missing entry
#pragma weak fdd_stiffness_matrix_lines_direct
#pragma weak fdd_csr_plan_gather_mapped
// and the coefficient instances of the line form (a diffusivity per point on a list whose unscaled factor blocks repeat,
// host/diffusivity.hpp): without them such a list streams its scaled arrays, and the flag "coefficient_in_kernel" refuses to be
// set to 1, naming the missing entry
#pragma weak fdd_stiffness_matrix_lines_coef
#pragma weak fdd_stiffness_matrix_lines_coef_f32
#pragma weak fdd_stiffness_matrix_lines_coef_direct
// and the mass, gradient and weak divergence of fields on the fine mesh (csrc/fdd_field.hip): without them the fddh_field_*
// entries refuse, naming the missing entry (missing_field_entry)
#pragma weak fdd_field_mass
#pragma weak fdd_field_gradient
#pragma weak fdd_field_weak_divergence
// and the convection term on the same mesh: without them fddh_convect and fddh_weak_convect refuse, naming the missing entry
// (missing_convect_entry)
#pragma weak fdd_field_convect
#pragma weak fdd_field_weak_convect
// and the zeroth-order term of a Helmholtz operator (csrc/fdd_helmholtz.hip): without them fddh_helmholtz_set refuses, naming
// the missing entry (missing_helmholtz_entry)
#pragma weak fdd_shift_add
#pragma weak fdd_shift_add_f32
#pragma weak fdd_shift_add_inner_product
// and the surface weights of boundary faces (csrc/fdd_field.hip): without it fddh_boundary_surface and fddh_boundary_robin_set
// refuse, naming the missing entry (missing_boundary_entry)
#pragma weak fdd_field_surface
// and the shift on the support of c alone: without them every shift runs the dense pass, and the flag "indexed_shift" refuses
// to be set to 1, naming the missing entry (missing_indexed_shift_entry)
#pragma weak fdd_shift_add_indexed
#pragma weak fdd_shift_add_indexed_f32
// and the last Arnoldi step of a cycle with its norm taken from the projections: without them that step keeps the exact pass,
// and the flag "last_norm_from_projections" refuses to be set to 1, naming the missing entry (missing_norm_estimate_entry)
#pragma weak fdd_multi_weighted_inner_product_self
#pragma weak fdd_multi_axpy_norm2_scaled_gated_dev
#pragma weak fdd_gmres_step_last_dev
#pragma weak fdd_gmres_fetch_norm_counters

namespace fdd
{

// the first entry the norm from the projections needs that the loaded kernel library does not export, or nullptr
inline const char *missing_norm_estimate_entry()
{
    if (&fdd_multi_weighted_inner_product_self == nullptr) return "fdd_multi_weighted_inner_product_self";
    if (&fdd_multi_axpy_norm2_scaled_gated_dev == nullptr) return "fdd_multi_axpy_norm2_scaled_gated_dev";
    if (&fdd_gmres_step_last_dev == nullptr) return "fdd_gmres_step_last_dev";
    if (&fdd_gmres_fetch_norm_counters == nullptr) return "fdd_gmres_fetch_norm_counters";
    return nullptr;
}

// the first entry a Robin coefficient needs beyond a Helmholtz shift's that the loaded kernel library does not export, or nullptr
inline const char *missing_boundary_entry()
{
    if (&fdd_field_surface == nullptr) return "fdd_field_surface";
    return nullptr;
}

inline const char *missing_indexed_shift_entry()
{
    if (&fdd_shift_add_indexed == nullptr) return "fdd_shift_add_indexed";
    if (&fdd_shift_add_indexed_f32 == nullptr) return "fdd_shift_add_indexed_f32";
    return nullptr;
}

// the first entry a Helmholtz shift needs that the loaded kernel library does not export (the mass matrix it is made from
// among them), or nullptr
inline const char *missing_helmholtz_entry()
{
    if (&fdd_shift_add == nullptr) return "fdd_shift_add";
    if (&fdd_shift_add_f32 == nullptr) return "fdd_shift_add_f32";
    if (&fdd_shift_add_inner_product == nullptr) return "fdd_shift_add_inner_product";
    if (&fdd_field_mass == nullptr) return "fdd_field_mass";
    return nullptr;
}

// the first of the field entries the loaded kernel library does not export, or nullptr
inline const char *missing_field_entry()
{
    if (&fdd_field_mass == nullptr) return "fdd_field_mass";
    if (&fdd_field_gradient == nullptr) return "fdd_field_gradient";
    if (&fdd_field_weak_divergence == nullptr) return "fdd_field_weak_divergence";
    return nullptr;
}

// the first of the convection entries the loaded kernel library does not export, or nullptr
inline const char *missing_convect_entry()
{
    if (&fdd_field_convect == nullptr) return "fdd_field_convect";
    if (&fdd_field_weak_convect == nullptr) return "fdd_field_weak_convect";
    return nullptr;
}

// the first AMG setup entry the loaded kernel library does not export, or nullptr
inline const char *missing_amg_setup_entry()
{
#define FDD_SETUP_ENTRY(name) {(const void *)&name, #name}
    const struct
    {
        const void *fn;
        const char *name;
    } entries[] = {FDD_SETUP_ENTRY(fdd_amg_setup_row_pointers), FDD_SETUP_ENTRY(fdd_amg_setup_spgemm_count),    FDD_SETUP_ENTRY(fdd_amg_setup_spgemm_fill),
                   FDD_SETUP_ENTRY(fdd_amg_setup_transpose_count), FDD_SETUP_ENTRY(fdd_amg_setup_transpose_fill), FDD_SETUP_ENTRY(fdd_amg_setup_fem_stencils),
                   FDD_SETUP_ENTRY(fdd_amg_setup_fem_count),    FDD_SETUP_ENTRY(fdd_amg_setup_fem_fill),        FDD_SETUP_ENTRY(fdd_amg_setup_inv_sqrt_diagonal),
                   FDD_SETUP_ENTRY(fdd_amg_setup_unit_values), FDD_SETUP_ENTRY(fdd_amg_setup_lattice_dofs), FDD_SETUP_ENTRY(fdd_amg_setup_lattice_coarse_flags), FDD_SETUP_ENTRY(fdd_amg_setup_lattice_cmap), FDD_SETUP_ENTRY(fdd_amg_setup_lattice_interp_count), FDD_SETUP_ENTRY(fdd_amg_setup_lattice_interp_fill), FDD_SETUP_ENTRY(fdd_amg_setup_lattice_coarse_points), FDD_SETUP_ENTRY(fdd_amg_setup_memory_info)};
#undef FDD_SETUP_ENTRY
    for (const auto &e : entries)
        if (e.fn == nullptr) return e.name;
    return nullptr;
}

// the first entry of the Chebyshev-Jacobi step the loaded kernel library does not export, or nullptr (fused: the gather's epilogue too)
inline const char *missing_chebyshev_entry(bool fused)
{
    if (&fdd_cheby_step == nullptr) return "fdd_cheby_step";
    if (&fdd_cheby_step_f32 == nullptr) return "fdd_cheby_step_f32";
    if (fused and &fdd_csr_plan_gather_cheby == nullptr) return "fdd_csr_plan_gather_cheby";
    if (fused and &fdd_csr_plan_gather_cheby_f32 == nullptr) return "fdd_csr_plan_gather_cheby_f32";
    return nullptr;
}

inline void check(int rc, const char *what)
{
    if (rc != 0)
    {
        fprintf(stderr, "ERROR: %s failed (code %d): %s\n", what, rc, fdd_last_error());
        exit(EXIT_FAILURE);
    }
}

#define FDD_CALL(expr) ::fdd::check((expr), #expr)

struct device_t
{
    void *stream = nullptr; // hipStream_t all kernels of this rank run on
    bool owns_stream = false; // created by fddh_init(own_stream): released by fddh_rank_finalize
    bool initialised = false; // fddh_init ran on this thread (a null stream alone cannot tell: it is also the legacy default stream)
    // which rank this is: a process-wide counter's next value, taken by the first fddh_init of the thread (and by the first
    // after an fddh_rank_finalize), 0 while the thread is no rank.  The address of this thread_local cannot serve: a thread
    // started after a rank thread has exited may get the same one.
    unsigned long long rank_instance = 0;

    template <typename T>
    class memory malloc(size_t n);

    void finish() { FDD_CALL(fdd_stream_sync(stream)); }
};

// the device handle of the calling rank: one rank = one host thread (the reference's model), so the state is
// thread_local and several ranks may live in one process (LocalComm, comm.hpp)
inline device_t &dev()
{
    static thread_local device_t d;
    return d;
}

// A block of fdd_malloc, given back when its last handle goes.  The deleter runs in destructors: a failed free prints one
// line and returns (FDD_CALL would exit).
inline std::shared_ptr<void> own_block(void *p)
{
    return std::shared_ptr<void>(p, [](void *q) {
        if (q != nullptr and fdd_free(q) != 0) fprintf(stderr, "WARNING: fdd_free failed: %s\n", fdd_last_error());
    });
}

// Shared ownership, as occa::memory: copies and slices share the block, so no view outlives its storage; free() means "this
// handle lets go".  A handle made from a raw pointer (owner = false) owns nothing.
class memory
{
  private:
    std::shared_ptr<void> block_;
    char *base_ = nullptr;
    size_t count_ = 0; // elements
    size_t elem_ = 1;  // bytes per element

    memory(std::shared_ptr<void> block, char *base, size_t count, size_t elem) : block_(std::move(block)), base_(base), count_(count), elem_(elem) {}

  public:
    memory() {}
    memory(void *p, size_t count, size_t elem, bool owner) : block_(owner ? own_block(p) : nullptr), base_((char *)p), count_(count), elem_(elem) {}

    void *ptr() const { return base_; }
    template <typename T>
    T *as() const
    {
        return reinterpret_cast<T *>(base_);
    }
    size_t size() const { return count_; }
    bool isInitialized() const { return base_ != nullptr; }

    // host -> device (blocking, like occa::memory::copyFrom(const void*, bytes))
    void copyFrom(const void *src, size_t bytes) { FDD_CALL(fdd_memcpy_h2d(base_, src, bytes, dev().stream)); }
    // device -> device
    void copyFrom(const memory &src, size_t bytes) { FDD_CALL(fdd_memcpy_d2d(base_, src.base_, bytes, dev().stream)); }
    // device -> host (blocking)
    void copyTo(void *dst, size_t bytes) const
    {
        if (bytes <= 256) // reduction results: pinned staging inside the library
            FDD_CALL(fdd_fetch_scalars(dst, base_, bytes, dev().stream));
        else
            FDD_CALL(fdd_memcpy_d2h(dst, base_, bytes, dev().stream));
    }
    // device -> device
    void copyTo(const memory &dst, size_t bytes) const { FDD_CALL(fdd_memcpy_d2d(dst.base_, base_, bytes, dev().stream)); }

    // element units, as occa::memory::slice(offset, count) (subdomain.tpp:3945-3946)
    memory slice(size_t offset, size_t count) const { return memory(block_, base_ + offset * elem_, count, elem_); }

    void free() { *this = memory(); }
};

template <typename T>
inline memory device_t::malloc(size_t n)
{
    void *p = nullptr;
    FDD_CALL(fdd_malloc(&p, n * sizeof(T)));
    return memory(p, n, sizeof(T), true);
}

// the one owner of a plan of fdd_csr_plan_create / _create_f32
struct csr_plan_deleter
{
    void operator()(fdd_csr_plan *p) const
    {
        if (fdd_csr_plan_destroy(p) != 0) fprintf(stderr, "WARNING: fdd_csr_plan_destroy failed: %s\n", fdd_last_error());
    }
};
using csr_plan = std::unique_ptr<fdd_csr_plan, csr_plan_deleter>;
inline csr_plan make_csr_plan(const int *ptr_hst, int num_rows, int num_cols, int num_nnz, bool f32 = false)
{
    fdd_csr_plan *p = nullptr;
    FDD_CALL((f32 ? fdd_csr_plan_create_f32 : fdd_csr_plan_create)(&p, ptr_hst, num_rows, num_cols, num_nnz));
    return csr_plan(p);
}

// Per-kernel timing with HIP events on the rank's own stream (what bench.py's
// `roofline` object reports).  Off by default; when on, two event records
// bracket each instrumented launch -- no synchronisation until collect().
// Keys are the device kernel families as rocprofv3 names them, so the averages
// can be checked against a --kernel-trace --stats run of the same command.
class KernelProfiler
{
  public:
    struct Stat
    {
        long long count = 0;
        double ms = 0.0;
        double bytes = 0.0; // algorithmic bytes, summed over launches
    };

  private:
    struct Rec
    {
        int key;
        double bytes;
        void *e0;
        void *e1;
    };
    std::vector<std::string> keys_;
    std::vector<Rec> recs_;
    std::vector<void *> pool_;
    size_t used_ = 0;

    void *event()
    {
        if (used_ == pool_.size())
        {
            void *e = nullptr;
            FDD_CALL(fdd_event_create(&e));
            pool_.push_back(e);
        }
        return pool_[used_++];
    }

    int key_id(const char *key)
    {
        for (size_t i = 0; i < keys_.size(); i++)
            if (keys_[i] == key) return (int)i;
        keys_.push_back(key);
        return (int)keys_.size() - 1;
    }

    std::vector<char> open_; // per open scope: was it recorded

  public:
    bool enabled = false;
    std::string only; // when set, only this kernel family is timed (two event records cost a few microseconds each)

    void begin(const char *key, double bytes)
    {
        if (!enabled) return;
        const bool take = only.empty() or only == key;
        open_.push_back(take ? 1 : 0);
        if (!take) return;
        Rec r{key_id(key), bytes, event(), event()};
        FDD_CALL(fdd_event_record(r.e0, dev().stream));
        recs_.push_back(r);
    }

    void end()
    {
        if (!enabled or open_.empty()) return;
        const bool took = open_.back() != 0;
        open_.pop_back();
        if (took) FDD_CALL(fdd_event_record(recs_.back().e1, dev().stream));
    }

    void reset()
    {
        recs_.clear();
        open_.clear();
        used_ = 0;
    }

    // synchronises, folds every recorded launch into per-key totals, clears
    std::vector<std::pair<std::string, Stat>> collect()
    {
        dev().finish();
        std::vector<Stat> stats(keys_.size());
        for (const Rec &r : recs_)
        {
            float ms = 0.0f;
            FDD_CALL(fdd_event_elapsed_ms(&ms, r.e0, r.e1));
            stats[r.key].count++;
            stats[r.key].ms += ms;
            stats[r.key].bytes += r.bytes;
        }
        reset();
        std::vector<std::pair<std::string, Stat>> out;
        for (size_t i = 0; i < keys_.size(); i++)
            if (stats[i].count) out.push_back(std::make_pair(keys_[i], stats[i]));
        return out;
    }
};

inline KernelProfiler &profiler()
{
    static thread_local KernelProfiler p;
    return p;
}

struct ProfileScope
{
    ProfileScope(const char *key, double bytes) { profiler().begin(key, bytes); }
    ~ProfileScope() { profiler().end(); }
};

} // namespace fdd

#endif
