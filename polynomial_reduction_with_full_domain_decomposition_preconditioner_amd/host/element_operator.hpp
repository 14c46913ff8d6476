/*
 * element_operator.hpp -- the element stiffness operator on one run of elements of one degree, stated once for the
 * Domain (which is exactly one such run) and the Subdomain (one run per polynomial level of its region): the list type,
 * the choice of kernel for the local form (Au = A_L u on element-local points) and for the gather form
 * (q = A_L (Q (s v)), Q read through an index array), and the check for affine elements.  This is the only host file that
 * names a stiffness entry of fdd_hip.h.  The profile labels and byte counts are the ones bench.py's kernel table keys on.
 */
#ifndef FDD_ELEMENT_OPERATOR_HPP
#define FDD_ELEMENT_OPERATOR_HPP

#include <algorithm>
#include <cstring>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "config.hpp"
#include "gll.hpp"

namespace fdd
{

template <typename Vec>
inline memory to_float(const Vec &v)
{
    std::vector<float> t(v.begin(), v.end());
    memory m = dev().malloc<float>(std::max<size_t>(t.size(), 1));
    if (not t.empty()) m.copyFrom(t.data(), t.size() * sizeof(float));
    return m;
}

// level-sorted element lists replace the per-point element / vertex / level / offset arrays of the reference
// (subdomain.tpp:1603-1630)
struct LevelList
{
    int level = 0;
    int poly_degree = 1;
    int dim = 3;
    int num_elements = 0;
    int first_offset = 0;                                                                      // the list is one run of elements, (N+1)^dim points apart from here
    const double *G[NUM_GEOM_FACTS] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; // geometric factors of the list's first point
    const double *D_hat = nullptr;                                                             // the degree's derivative table (its owner rewrites it in place: Domain::set_D_hat)
    // float copies for the single-precision inner solve (Subdomain::prepare_single_precision); not allocated before
    memory G32[NUM_GEOM_FACTS], D_hat32;
    // affine elements (an option, set_affine_geometry): six numbers per element + the GLL weights stand for the factor arrays
    bool affine = false;            // in use
    double affine_deviation = -1.0; // largest relative deviation found (-1: not checked)
    memory affine_c, affine_w, affine_c32, affine_w32;
    // are the three off-diagonal factor arrays G[3..5] zero at every point of the list (detect_zero_factors, once, when the
    // factor pointers are set)?  Then the kernel that does not stream them applies; G32 are casts of the same arrays
    bool offdiag_zero = false;
    // do the list's elements share their G[0..2] blocks with a few representatives, bit for bit (detect_shared_blocks, once,
    // after the check above)?  factor_elem[e]: the lowest element of the list that holds element e's block; G32 are casts
    // of the same arrays, so equal double blocks are equal float blocks and the one map serves both precisions
    bool shared_blocks = false;
    int factor_classes = 0; // distinct blocks found (0: not looked for)
    memory factor_elem;     // device ints, allocated only where shared_blocks holds
    // does the table behind D_hat / D_hat32 meet the lean line instance's conditions (check_lean_table, on the host array
    // each upload is made from; each precision on its own)?
    bool lean_D_hat = false, lean_D_hat32 = false;

    size_t num_points() const { return (size_t)num_elements * (poly_degree + 1) * (poly_degree + 1) * (dim == 3 ? poly_degree + 1 : 1); }
};

// the matrix-core kernels exist in double only, for 3-D elements of degree 11..15
template <typename Real>
inline bool on_matrix_cores(const LevelList &ll, bool mfma_enabled)
{
    return std::is_same<Real, double>::value and mfma_enabled and ll.dim == 3 and ll.poly_degree >= 11 and ll.poly_degree <= 15;
}

// the first entry of the three-array stiffness kernel the loaded kernel library does not export, or nullptr
inline const char *missing_zero_factor_entry()
{
    if (&fdd_stiffness_offdiag_zero == nullptr) return "fdd_stiffness_offdiag_zero";
    if (&fdd_stiffness_matrix_diag == nullptr) return "fdd_stiffness_matrix_diag";
    if (&fdd_stiffness_matrix_diag_f32 == nullptr) return "fdd_stiffness_matrix_diag_f32";
    return nullptr;
}

// the entry of the matrix-core kernel on three factor arrays, where the loaded kernel library does not export it, or nullptr
inline const char *missing_mfma_zero_factor_entry()
{
    if (&fdd_stiffness_matrix_mfma_diag == nullptr) return "fdd_stiffness_matrix_mfma_diag";
    return missing_zero_factor_entry(); // the check that sets LevelList::offdiag_zero
}

// ---- factor arrays that are identically zero (flag "skip_zero_factors") ----
// On a mesh whose elements have orthogonal axes (every box, every rectilinear grid) G[3..5] are 0.0 at every point.
// detect_zero_factors establishes that from the list's OWN arrays in one pass on the device; where it holds (and the flag
// is on) the list runs the kernel that streams G[0..2] only.  Unlike the affine option the arithmetic left out is the
// addition of exact zeros: the operator's values are the same, to the sign of a zero.  Only 3-D lists of degree <= 15 are
// checked (the 2-D and two-launch forms keep six arrays); without the entries nothing is, and nothing switches.  A list that
// runs on the matrix cores takes their three-array instance (on_mfma_diag_kernel, flag "mfma_skip_zero_factors").
inline void detect_zero_factors(LevelList &ll)
{
    ll.offdiag_zero = false;
    if (ll.dim != 3 or ll.poly_degree > 15 or ll.num_elements == 0 or missing_zero_factor_entry()) return;
    int flags[3] = {1, 1, 1};
    memory flags_dev = dev().malloc<int>(3);
    FDD_CALL(fdd_stiffness_offdiag_zero(flags_dev.as<int>(), ll.G, nullptr, ll.num_elements, ll.poly_degree, dev().stream));
    flags_dev.copyTo(flags, sizeof(flags));
    flags_dev.free();
    ll.offdiag_zero = flags[0] == 0 and flags[1] == 0 and flags[2] == 0;
}

// does the list run the three-array kernel for this precision?  (affine, where switched on, takes precedence: see the callers)
template <typename Real>
inline bool on_diag_kernel(const LevelList &ll, bool mfma_enabled, bool skip_zero_factors)
{
    return skip_zero_factors and ll.offdiag_zero and not ll.affine and not on_matrix_cores<Real>(ll, mfma_enabled);
}

// does the list run the matrix-core kernel on three factor arrays?  Both flags: "skip_zero_factors" = 0 goes on meaning six
// arrays everywhere.  The values are those of the six-array matrix-core kernel, to the sign of a zero.
template <typename Real>
inline bool on_mfma_diag_kernel(const LevelList &ll, bool mfma_enabled, bool skip_zero_factors, bool mfma_skip_zero_factors)
{
    return on_matrix_cores<Real>(ll, mfma_enabled) and skip_zero_factors and mfma_skip_zero_factors and ll.offdiag_zero and not ll.affine and missing_mfma_zero_factor_entry() == nullptr;
}

// ---- the line form of the stiffness kernel (flag "line_stiffness") ----
// the first entry of the line form the loaded kernel library does not export, or nullptr
inline const char *missing_line_stiffness_entry()
{
    if (&fdd_stiffness_matrix_lines == nullptr) return "fdd_stiffness_matrix_lines";
    if (&fdd_stiffness_matrix_lines_f32 == nullptr) return "fdd_stiffness_matrix_lines_f32";
    return nullptr;
}

// does the list run the line form for this precision, in the local and in the gather form alike?  3-D, degree 7 (an element
// is one wavefront), not affine, not on the matrix cores, entry present, flag on -- and on the three-array kernel
// (on_diag_kernel): the six-array line form measured no faster than the slab form in either precision (172.9 against 169.7
// and 94.2 against 93.6 us per launch at 32^3 elements), so those lists keep the slab form and the kernel library compiles
// no six-array line instance.  The line form gives the bits of the instance it replaces, so nothing that hangs on the
// operator changes with the flag.
template <typename Real>
inline bool on_line_kernel(const LevelList &ll, bool mfma_enabled, bool skip_zero_factors, bool line_stiffness)
{
    return line_stiffness and ll.dim == 3 and ll.poly_degree == 7 and on_diag_kernel<Real>(ll, mfma_enabled, skip_zero_factors) and missing_line_stiffness_entry() == nullptr;
}

// ---- factor blocks that repeat from element to element (flag "shared_factor_blocks") ----
// the first entry of the shared-block line instance and its detection the loaded kernel library does not export, or nullptr
inline const char *missing_shared_factor_entry()
{
    if (&fdd_stiffness_matrix_lines_shared == nullptr) return "fdd_stiffness_matrix_lines_shared";
    if (&fdd_stiffness_matrix_lines_shared_f32 == nullptr) return "fdd_stiffness_matrix_lines_shared_f32";
    if (&fdd_stiffness_factor_block_hash == nullptr) return "fdd_stiffness_factor_block_hash";
    if (&fdd_stiffness_factor_block_verify == nullptr) return "fdd_stiffness_factor_block_verify";
    return nullptr;
}

// The distinct blocks of a shared list occupy at most this many bytes (85 of them at degree 7): a quarter of the 4 MiB of
// L2 of one XCD, so that they stay there beside the streamed vectors.  A design bound from the cache size, not a tuned value.
constexpr size_t shared_factor_bytes_limit = (size_t)1 << 20;

// On a mesh whose elements are translated copies of a few shapes (a uniform box, a piecewise-uniform grid) every element's
// block of G[0..2] is bit for bit the block of one of a few elements, and the line kernel's shared instance reads that one
// instead of streaming the copies.  Established from the list's OWN arrays, once, like detect_zero_factors (the factor arrays
// are written at initialisation and never in place afterwards): a hash per element on the device, equal hashes grouped on
// the host with the lowest element as representative, then every element compared with its representative bit by bit on
// the device -- a hash collision makes the list not shared, it never reaches the operator.  Shared: verified, the distinct
// blocks within shared_factor_bytes_limit, and at most half as many of them as elements (the factor stream at least halves).
// Only lists with offdiag_zero are looked at; a deformed mesh pays one pass over three arrays and stays as it is.
inline void detect_shared_blocks(LevelList &ll)
{
    ll.shared_blocks = false;
    ll.factor_classes = 0;
    ll.factor_elem.free();
    if (not ll.offdiag_zero or ll.dim != 3 or ll.poly_degree > 15 or ll.num_elements == 0 or missing_shared_factor_entry()) return;
    const size_t ne = (size_t)ll.num_elements;
    std::vector<unsigned long long> hash(ne);
    memory hash_dev = dev().malloc<unsigned long long>(ne);
    FDD_CALL(fdd_stiffness_factor_block_hash(hash_dev.as<unsigned long long>(), ll.G, nullptr, ll.num_elements, ll.poly_degree, dev().stream));
    hash_dev.copyTo(hash.data(), ne * sizeof(unsigned long long));
    hash_dev.free();
    std::vector<int> rep(ne);
    std::unordered_map<unsigned long long, int> first; // elements in ascending order: the first of a group is its lowest
    for (size_t e = 0; e < ne; e++) rep[e] = first.emplace(hash[e], (int)e).first->second;
    ll.factor_classes = (int)first.size();
    const size_t block_bytes = 3 * (ll.num_points() / ne) * sizeof(double);
    if (first.size() * block_bytes > shared_factor_bytes_limit or 2 * first.size() > ne) return;
    int mismatches = 1;
    memory rep_dev = dev().malloc<int>(ne), mismatches_dev = dev().malloc<int>(1);
    rep_dev.copyFrom(rep.data(), ne * sizeof(int));
    FDD_CALL(fdd_stiffness_factor_block_verify(mismatches_dev.as<int>(), ll.G, nullptr, rep_dev.as<int>(), ll.num_elements, ll.poly_degree, dev().stream));
    mismatches_dev.copyTo(&mismatches, sizeof(int));
    mismatches_dev.free();
    if (mismatches != 0)
    {
        rep_dev.free();
        return;
    }
    ll.factor_elem = rep_dev;
    ll.shared_blocks = true;
}

// does the list run the shared instance of the line form?  Only where it runs the line form at all, so every flag and
// condition on_line_kernel looks at keeps its meaning and precedence.  Same bits as the streamed instance.
template <typename Real>
inline bool on_shared_line_kernel(const LevelList &ll, bool mfma_enabled, bool skip_zero_factors, bool line_stiffness, bool shared_factor_blocks)
{
    return shared_factor_blocks and ll.shared_blocks and on_line_kernel<Real>(ll, mfma_enabled, skip_zero_factors, line_stiffness) and missing_shared_factor_entry() == nullptr;
}

// ---- the lean instances of the line form (flag "lean_line_stiffness") ----
// the first entry of the lean line instances the loaded kernel library does not export, or nullptr
inline const char *missing_lean_line_entry()
{
    if (&fdd_stiffness_matrix_lines_lean == nullptr) return "fdd_stiffness_matrix_lines_lean";
    if (&fdd_stiffness_matrix_lines_lean_f32 == nullptr) return "fdd_stiffness_matrix_lines_lean_f32";
    return nullptr;
}

// What fdd_stiffness_matrix_lines_lean[_f32] asks of an 8 x 8 table, bit for bit: the interior diagonal is +-0.0 (either
// sign, each entry on its own: gll::dgll writes +0.0 on all six) and everywhere else entry 63 - m has the bits of the negation
// of entry m.  A NaN passes only with its mirror image's payload and the other sign.
template <typename Real>
inline bool lean_table_ok(const Real *D)
{
    using Bits = typename std::conditional<sizeof(Real) == 8, unsigned long long, unsigned int>::type;
    const Bits sign = (Bits)1 << (8 * sizeof(Real) - 1);
    Bits w[64];
    memcpy(w, D, sizeof(w));
    for (int i = 1; i <= 6; i++)
        if ((w[9 * i] & ~sign) != 0) return false;
    for (int m = 0; m < 32; m++)
        if (m != 9 and m != 18 and m != 27 and w[63 - m] != (w[m] ^ sign)) return false;
    return true;
}

// The float table is the cast to_float makes of the double one when the single-precision inner solve is prepared
// (Subdomain::prepare_single_precision) and is not remade afterwards: the verdict on it follows the same rule.
inline void check_lean_table32(LevelList &ll, const std::vector<double> &D)
{
    const std::vector<float> D32(D.begin(), D.end());
    ll.lean_D_hat32 = ll.poly_degree == 7 and D32.size() == 64 and lean_table_ok(D32.data());
}

// Called wherever a list's double table is uploaded (set-up, set_D_hat), with the host array the upload is made from.
// Tables of other sizes fail.  While no float copy exists yet the verdict on it is that of the cast it would be made from.
inline void check_lean_table(LevelList &ll, const std::vector<double> &D)
{
    ll.lean_D_hat = ll.poly_degree == 7 and D.size() == 64 and lean_table_ok(D.data());
    if (not ll.D_hat32.ptr()) check_lean_table32(ll, D);
}

// does the list run a lean instance of the line form (shared where on_shared_line_kernel holds, streamed otherwise)?  Only
// where it runs the line form at all and its table in this precision passed the check; a table that did not keeps the parent
// instance.  The parent's values, to the sign of a zero.
template <typename Real>
inline bool on_lean_line_kernel(const LevelList &ll, bool mfma_enabled, bool skip_zero_factors, bool line_stiffness, bool lean_line_stiffness)
{
    return lean_line_stiffness and (std::is_same<Real, float>::value ? ll.lean_D_hat32 : ll.lean_D_hat) and on_line_kernel<Real>(ll, mfma_enabled, skip_zero_factors, line_stiffness) and missing_lean_line_entry() == nullptr;
}

// Au = A_L u on the points of the list (Au, u: the vectors the list's first_offset counts in).  workspace: three vectors
// of the list's points for the two-launch form above degree 15.
inline void apply_local(const LevelList &ll, double *Au, const double *u, const std::vector<memory> &workspace, bool mfma_enabled, bool skip_zero_factors, bool line_stiffness, bool mfma_skip_zero_factors, bool shared_factor_blocks, bool lean_line_stiffness)
{
    void *stream = dev().stream;
    const double points = (double)ll.num_points();
    Au += ll.first_offset, u += ll.first_offset;
    if (on_mfma_diag_kernel<double>(ll, mfma_enabled, skip_zero_factors, mfma_skip_zero_factors) and Au != u)
    {
        // not "mfma_stiffness_kernel...": the committed counters bench.py matches by that prefix are the six-array kernel's
        ProfileScope prof("mfma_diag_stiffness_kernel", 40.0 * points);
        FDD_CALL(fdd_stiffness_matrix_mfma_diag(Au, u, nullptr, nullptr, ll.D_hat, ll.G, nullptr, ll.num_elements, ll.poly_degree, stream));
    }
    else if (on_matrix_cores<double>(ll, mfma_enabled) and Au != u)
    {
        // high order: the six contractions on the fp64 matrix cores (tolerance-level parity, fdd_hip.h)
        ProfileScope prof("mfma_stiffness_kernel", 64.0 * points);
        FDD_CALL(fdd_stiffness_matrix_mfma(Au, u, ll.D_hat, ll.G, nullptr, ll.num_elements, ll.poly_degree, stream));
    }
    else if (on_lean_line_kernel<double>(ll, mfma_enabled, skip_zero_factors, line_stiffness, lean_line_stiffness))
    {
        const bool shared = on_shared_line_kernel<double>(ll, mfma_enabled, skip_zero_factors, line_stiffness, shared_factor_blocks);
        ProfileScope prof(shared ? "line_stiffness_kernel<shared,lean>" : "line_stiffness_kernel<lean>", (shared ? 16.0 : 40.0) * points); // the bytes of the parent instance
        FDD_CALL(fdd_stiffness_matrix_lines_lean(Au, u, nullptr, nullptr, ll.D_hat, ll.G, nullptr, shared ? ll.factor_elem.as<int>() : nullptr, ll.num_elements, ll.poly_degree, 1, stream));
    }
    else if (on_shared_line_kernel<double>(ll, mfma_enabled, skip_zero_factors, line_stiffness, shared_factor_blocks))
    {
        ProfileScope prof("line_stiffness_kernel<shared>", 16.0 * points); // u and Au; the few factor blocks stay in cache
        FDD_CALL(fdd_stiffness_matrix_lines_shared(Au, u, nullptr, nullptr, ll.D_hat, ll.G, nullptr, ll.factor_elem.as<int>(), ll.num_elements, ll.poly_degree, 1, stream));
    }
    else if (on_line_kernel<double>(ll, mfma_enabled, skip_zero_factors, line_stiffness))
    {
        ProfileScope prof("line_stiffness_kernel", 40.0 * points); // the bytes of the three-array instance it replaces
        FDD_CALL(fdd_stiffness_matrix_lines(Au, u, nullptr, nullptr, ll.D_hat, ll.G, nullptr, ll.num_elements, ll.poly_degree, 1, stream));
    }
    else if (on_diag_kernel<double>(ll, mfma_enabled, skip_zero_factors)) // the gather form's predicate: one answer per list (3-D, degree <= 15: nothing else is checked)
    {
        // the labels of the three-array instances are not "fused_stiffness_kernel...": the committed counters bench.py
        // matches by family are the six-array kernel's
        ProfileScope prof("diag_stiffness_kernel", 40.0 * points);
        FDD_CALL(fdd_stiffness_matrix_diag(Au, u, nullptr, nullptr, ll.D_hat, ll.G, nullptr, ll.num_elements, ll.poly_degree, stream));
    }
    else if (ll.dim == 3 and ll.poly_degree <= 15)
    {
        ProfileScope prof("fused_stiffness_kernel", 64.0 * points);
        FDD_CALL(fdd_sub_stiffness_matrix(Au, u, ll.D_hat, ll.G, nullptr, ll.num_elements, ll.poly_degree, stream));
    }
    else if (ll.dim == 2 and ll.poly_degree <= 15)
    {
        ProfileScope prof("fused_stiffness_2d_kernel", 40.0 * points);
        FDD_CALL(fdd_stiffness_matrix_2d(Au, u, ll.D_hat, ll.G, nullptr, ll.num_elements, ll.poly_degree, stream));
    }
    else
    {
        // degree above 15: the reference's two-launch form (domain.tpp:605-606) on the list
        double *GDu[3] = {workspace[0].as<double>(), workspace[1].as<double>(), workspace[2].as<double>()};
        FDD_CALL(fdd_dom_stiffness_matrix_1(GDu, u, ll.D_hat, ll.G, (int)ll.num_points(), ll.poly_degree, ll.dim, stream));
        FDD_CALL(fdd_dom_stiffness_matrix_2(Au, GDu, ll.D_hat, (int)ll.num_points(), ll.poly_degree, ll.dim, stream));
    }
}

namespace ops
{
// the gather entries per precision, as in precision_ops.hpp; q, point_index: at the list's first point
inline void stiffness_gather(const LevelList &ll, double *q, const double *v, const double *scale_dev, const int *point_index, bool mfma, void *s)
{
    FDD_CALL((mfma ? fdd_stiffness_matrix_mfma_gather : fdd_sub_stiffness_matrix_gather_scaled)(q, v, scale_dev, point_index, ll.D_hat, ll.G, nullptr, ll.num_elements, ll.poly_degree, s));
}
inline void stiffness_gather(const LevelList &ll, float *q, const float *v, const double *scale_dev, const int *point_index, bool, void *s)
{
    const float *G[NUM_GEOM_FACTS];
    for (int g = 0; g < NUM_GEOM_FACTS; g++) G[g] = ll.G32[g].as<float>();
    FDD_CALL(fdd_sub_stiffness_matrix_gather_scaled_f32(q, v, scale_dev, point_index, ll.D_hat32.as<float>(), G, nullptr, ll.num_elements, ll.poly_degree, s));
}
inline void stiffness_diag(const LevelList &ll, double *q, const double *v, const double *scale_dev, const int *point_index, void *s)
{
    FDD_CALL(fdd_stiffness_matrix_diag(q, v, scale_dev, point_index, ll.D_hat, ll.G, nullptr, ll.num_elements, ll.poly_degree, s));
}
inline void stiffness_diag(const LevelList &ll, float *q, const float *v, const double *scale_dev, const int *point_index, void *s)
{
    const float *G[NUM_GEOM_FACTS];
    for (int g = 0; g < NUM_GEOM_FACTS; g++) G[g] = ll.G32[g].as<float>();
    FDD_CALL(fdd_stiffness_matrix_diag_f32(q, v, scale_dev, point_index, ll.D_hat32.as<float>(), G, nullptr, ll.num_elements, ll.poly_degree, s));
}
inline void stiffness_mfma_diag(const LevelList &ll, double *q, const double *v, const double *scale_dev, const int *point_index, void *s)
{
    FDD_CALL(fdd_stiffness_matrix_mfma_diag(q, v, scale_dev, point_index, ll.D_hat, ll.G, nullptr, ll.num_elements, ll.poly_degree, s));
}
inline void stiffness_lines(const LevelList &ll, double *q, const double *v, const double *scale_dev, const int *point_index, void *s)
{
    FDD_CALL(fdd_stiffness_matrix_lines(q, v, scale_dev, point_index, ll.D_hat, ll.G, nullptr, ll.num_elements, ll.poly_degree, 1, s));
}
inline void stiffness_lines(const LevelList &ll, float *q, const float *v, const double *scale_dev, const int *point_index, void *s)
{
    const float *G[NUM_GEOM_FACTS];
    for (int g = 0; g < NUM_GEOM_FACTS; g++) G[g] = ll.G32[g].as<float>();
    FDD_CALL(fdd_stiffness_matrix_lines_f32(q, v, scale_dev, point_index, ll.D_hat32.as<float>(), G, nullptr, ll.num_elements, ll.poly_degree, 1, s));
}
inline void stiffness_lines_shared(const LevelList &ll, double *q, const double *v, const double *scale_dev, const int *point_index, void *s)
{
    FDD_CALL(fdd_stiffness_matrix_lines_shared(q, v, scale_dev, point_index, ll.D_hat, ll.G, nullptr, ll.factor_elem.as<int>(), ll.num_elements, ll.poly_degree, 1, s));
}
inline void stiffness_lines_shared(const LevelList &ll, float *q, const float *v, const double *scale_dev, const int *point_index, void *s)
{
    const float *G[NUM_GEOM_FACTS];
    for (int g = 0; g < NUM_GEOM_FACTS; g++) G[g] = ll.G32[g].as<float>();
    FDD_CALL(fdd_stiffness_matrix_lines_shared_f32(q, v, scale_dev, point_index, ll.D_hat32.as<float>(), G, nullptr, ll.factor_elem.as<int>(), ll.num_elements, ll.poly_degree, 1, s));
}
inline void stiffness_lines_lean(const LevelList &ll, double *q, const double *v, const double *scale_dev, const int *point_index, bool shared, void *s)
{
    FDD_CALL(fdd_stiffness_matrix_lines_lean(q, v, scale_dev, point_index, ll.D_hat, ll.G, nullptr, shared ? ll.factor_elem.as<int>() : nullptr, ll.num_elements, ll.poly_degree, 1, s));
}
inline void stiffness_lines_lean(const LevelList &ll, float *q, const float *v, const double *scale_dev, const int *point_index, bool shared, void *s)
{
    const float *G[NUM_GEOM_FACTS];
    for (int g = 0; g < NUM_GEOM_FACTS; g++) G[g] = ll.G32[g].as<float>();
    FDD_CALL(fdd_stiffness_matrix_lines_lean_f32(q, v, scale_dev, point_index, ll.D_hat32.as<float>(), G, nullptr, shared ? ll.factor_elem.as<int>() : nullptr, ll.num_elements, ll.poly_degree, 1, s));
}
inline void stiffness_affine(const LevelList &ll, double *q, const double *v, const double *scale_dev, const int *point_index, bool mfma, void *s)
{
    FDD_CALL((mfma ? fdd_stiffness_matrix_mfma_affine : fdd_stiffness_matrix_affine)(q, v, scale_dev, point_index, ll.D_hat, ll.affine_c.as<double>(), ll.affine_w.as<double>(), nullptr, ll.num_elements, ll.poly_degree, s));
}
inline void stiffness_affine(const LevelList &ll, float *q, const float *v, const double *scale_dev, const int *point_index, bool, void *s)
{
    FDD_CALL(fdd_stiffness_matrix_affine_f32(q, v, scale_dev, point_index, ll.D_hat32.as<float>(), ll.affine_c32.as<float>(), ll.affine_w32.as<float>(), nullptr, ll.num_elements, ll.poly_degree, s));
}
}

// q (points of the list) = A_L (Q (s v)): u[p] = s v[point_index[p]] on load (0 where the index is negative), s = *scale_dev
// (null: 1).  q, point_index: the arrays the list's first_offset counts in; gathered_values: the length of v (the bytes it
// adds to the count).  3-D lists of degree <= 15.
template <typename Real>
inline void apply_gather(const LevelList &ll, Real *q, const Real *v, const int *point_index, const double *scale_dev, int gathered_values, bool mfma_enabled, bool skip_zero_factors, bool line_stiffness, bool mfma_skip_zero_factors, bool shared_factor_blocks, bool lean_line_stiffness)
{
    constexpr bool f32 = std::is_same<Real, float>::value;
    const bool mfma = on_matrix_cores<Real>(ll, mfma_enabled);
    const double points = (double)ll.num_points(), gathered = (double)sizeof(Real) * gathered_values;
    q += ll.first_offset, point_index += ll.first_offset;
    if (ll.affine)
    {
        ProfileScope prof(f32 ? "fused_stiffness_kernel<gather,f32,affine>" : mfma ? "mfma_stiffness_kernel<gather,affine>" : "fused_stiffness_kernel<gather,affine>", (f32 ? 8.0 : 12.0) * points + gathered);
        ops::stiffness_affine(ll, q, v, scale_dev, point_index, mfma, dev().stream);
        return;
    }
    if constexpr (not f32) // the matrix-core kernels exist in double only
        if (on_mfma_diag_kernel<Real>(ll, mfma_enabled, skip_zero_factors, mfma_skip_zero_factors))
        {
            ProfileScope prof("mfma_diag_stiffness_kernel<gather>", 36.0 * points + gathered);
            ops::stiffness_mfma_diag(ll, q, v, scale_dev, point_index, dev().stream);
            return;
        }
    if (on_lean_line_kernel<Real>(ll, mfma_enabled, skip_zero_factors, line_stiffness, lean_line_stiffness))
    {
        const bool shared = on_shared_line_kernel<Real>(ll, mfma_enabled, skip_zero_factors, line_stiffness, shared_factor_blocks);
        const char *label = shared ? (f32 ? "line_stiffness_kernel<gather,shared,f32,lean>" : "line_stiffness_kernel<gather,shared,lean>") : (f32 ? "line_stiffness_kernel<gather,f32,lean>" : "line_stiffness_kernel<gather,lean>");
        ProfileScope prof(label, (shared ? (f32 ? 8.0 : 12.0) : (f32 ? 20.0 : 36.0)) * points + gathered); // the bytes of the parent instance
        ops::stiffness_lines_lean(ll, q, v, scale_dev, point_index, shared, dev().stream);
        return;
    }
    if (on_shared_line_kernel<Real>(ll, mfma_enabled, skip_zero_factors, line_stiffness, shared_factor_blocks))
    {
        ProfileScope prof(f32 ? "line_stiffness_kernel<gather,shared,f32>" : "line_stiffness_kernel<gather,shared>", (f32 ? 8.0 : 12.0) * points + gathered); // index and q; the few factor blocks stay in cache
        ops::stiffness_lines_shared(ll, q, v, scale_dev, point_index, dev().stream);
        return;
    }
    if (on_line_kernel<Real>(ll, mfma_enabled, skip_zero_factors, line_stiffness))
    {
        ProfileScope prof(f32 ? "line_stiffness_kernel<gather,f32>" : "line_stiffness_kernel<gather>", (f32 ? 20.0 : 36.0) * points + gathered); // the bytes of the instance it replaces
        ops::stiffness_lines(ll, q, v, scale_dev, point_index, dev().stream);
        return;
    }
    if (on_diag_kernel<Real>(ll, mfma_enabled, skip_zero_factors))
    {
        ProfileScope prof(f32 ? "diag_stiffness_kernel<gather,f32>" : "diag_stiffness_kernel<gather>", (f32 ? 20.0 : 36.0) * points + gathered);
        ops::stiffness_diag(ll, q, v, scale_dev, point_index, dev().stream);
        return;
    }
    ProfileScope prof(f32 ? "fused_stiffness_kernel<gather,f32>" : mfma ? "mfma_stiffness_kernel<gather>" : "fused_stiffness_kernel<gather>", (f32 ? 32.0 : 60.0) * points + gathered);
    ops::stiffness_gather(ll, q, v, scale_dev, point_index, mfma, dev().stream);
}

// ---- affine elements (an option of this build; the reference always streams the six factor arrays) ----
// Where an element is an affine image of the reference cube, the factors of a point are c_f(e) (w_i w_j) w_k: the kernel
// forms them from six numbers per element and does not read 48 of its 64 bytes per point.  detect_affine checks the list's
// OWN factor arrays against that form on the device, once (the deviation is kept), and says whether every element passes.
// A list that cannot run the affine kernel (not 3-D, degree above 15, no elements) is not checked.
constexpr double affine_tolerance = 64.0 * 2.220446049250313e-16;
inline bool detect_affine(LevelList &ll)
{
    if (ll.dim != 3 or ll.poly_degree > 15 or ll.num_elements == 0) return false;
    if (ll.affine_deviation < 0.0)
    {
        const int n = ll.poly_degree + 1;
        std::vector<double> z(n), w(n), dev_hst(ll.num_elements);
        gll::zwgll(z.data(), w.data(), n);
        ll.affine_w = dev().malloc<double>(n);
        ll.affine_w.copyFrom(w.data(), (size_t)n * sizeof(double));
        ll.affine_c = dev().malloc<double>((size_t)ll.num_elements * NUM_GEOM_FACTS);
        memory dev_dev = dev().malloc<double>(ll.num_elements);
        FDD_CALL(fdd_stiffness_affine_detect(ll.affine_c.as<double>(), dev_dev.as<double>(), ll.G, nullptr, ll.affine_w.as<double>(), ll.num_elements, ll.poly_degree, dev().stream));
        dev_dev.copyTo(dev_hst.data(), dev_hst.size() * sizeof(double));
        dev_dev.free();
        ll.affine_deviation = 0.0;
        for (double x : dev_hst) ll.affine_deviation = (x == x) ? std::max(ll.affine_deviation, x) : 1.0;
    }
    return ll.affine_deviation <= affine_tolerance;
}

// the float copies of a checked list's element factors and weights, made when first asked for (the single-precision
// inner solve reads them; a Domain never asks)
inline void affine_float_copies(LevelList &ll)
{
    if (ll.affine_deviation < 0.0 or ll.affine_c32.ptr()) return;
    const int n = ll.poly_degree + 1;
    std::vector<double> z(n), w(n), c_hst((size_t)ll.num_elements * NUM_GEOM_FACTS);
    gll::zwgll(z.data(), w.data(), n);
    ll.affine_c.copyTo(c_hst.data(), c_hst.size() * sizeof(double));
    ll.affine_c32 = to_float(c_hst);
    ll.affine_w32 = to_float(w);
}

} // namespace fdd

#endif
