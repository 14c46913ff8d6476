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
#include <array>
#include <cstring>
#include <stdexcept>
#include <string>
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
    bool affine = false;            // in use; only 3-D lists of degree <= 15 (detect_affine checks no other)
    bool affine_requested = false;  // the option as last asked for: a list whose arrays are rewritten is checked again (diffusivity.hpp)
    double affine_deviation = -1.0; // largest relative deviation found (-1: not checked)
    memory affine_c, affine_w, affine_c32, affine_w32;
    // are the three off-diagonal factor arrays G[3..5] zero at every point of the list (detect_zero_factors, once, when the
    // factor pointers are set)?  Then the kernel that does not stream them applies; G32 are casts of the same arrays.
    // Only 3-D lists of degree <= 15
    bool offdiag_zero = false;
    // do the list's elements share their G[0..2] blocks with a few representatives, bit for bit (detect_shared_blocks, once,
    // after the check above)?  factor_elem[e]: the lowest element of the list that holds element e's block; G32 are casts
    // of the same arrays, so equal double blocks are equal float blocks and the one map serves both precisions.
    // Only with offdiag_zero
    bool shared_blocks = false;
    int factor_classes = 0; // distinct blocks found (0: not looked for)
    memory factor_elem;     // device ints, allocated only where shared_blocks holds
    // does the table behind D_hat / D_hat32 meet the lean line instance's conditions (check_lean_table, on the host array
    // each upload is made from; each precision on its own)?  Only at degree 7
    bool lean_D_hat = false, lean_D_hat32 = false;
    // a diffusivity per point is set (diffusivity.hpp): G and G32 then hold the scaled arrays kappa G, which every kernel
    // reads as it reads the mesh's own.  Where the list is 3-D of degree 7 and its UNSCALED arrays shared blocks (the verdict
    // of detect_shared_blocks on the mesh's arrays, kept by diffusivity.hpp), the coefficient line instance can form kappa G
    // itself (flag "coefficient_in_kernel"): coef, device doubles per point; coef_blocks, the distinct unscaled blocks of
    // G[0..2] in compact form (block c at c (N+1)^3); coef_block_of_elem, device ints per element.  Not allocated otherwise
    memory coef, coef_blocks[3], coef_block_of_elem;

    size_t num_points() const { return (size_t)num_elements * (poly_degree + 1) * (poly_degree + 1) * (dim == 3 ? poly_degree + 1 : 1); }
};

// ---- the flags that choose between the stiffness kernels ----
// One value per Domain and per Subdomain.  A flag is on by default where the loaded kernel library exports the flag's
// entries, and set_stiffness_flag refuses to turn on one whose entries are missing: that function is the only place that
// keeps "a flag that is on has its entries", and choose_stiffness below relies on it without asking the weak symbols.
// None of the flags empties anything that hangs on the operator (projection basis, point-Jacobi diagonal, Chebyshev bound):
struct StiffnessFlags
{
    // 3-D lists of degree 11..15 run on the fp64 matrix cores, in double (tolerance-level parity, fdd_hip.h); no entry is
    // asked for: the matrix-core six-array entries are not weak
    bool mfma_stiffness;
    // lists whose three off-diagonal factor arrays are zero at every point (detect_zero_factors) run the kernel that streams
    // three arrays; 0: six arrays everywhere.  The operator's values do not change -- what is left out is the addition of
    // exact zeros -- so the projection basis, the point-Jacobi diagonal and the Chebyshev bound stay
    bool skip_zero_factors;
    // the same for lists on the matrix cores: their three-array instance, while "skip_zero_factors" and "mfma_stiffness"
    // are both on; 0: those lists stream six arrays.  The values are the six-array matrix-core kernel's, to the sign of a
    // zero, so nothing is emptied here either
    bool mfma_skip_zero_factors;
    // 3-D degree-7 lists on the three-array kernel run its line form (an element is one wavefront); 0: the slab form.  The
    // six-array line form measured no faster than the slab form in either precision (172.9 against 169.7 and 94.2 against
    // 93.6 us per launch at 32^3 elements), so those lists keep the slab form and the kernel library compiles no six-array
    // line instance.  Same bits either way, so nothing that hangs on the operator is emptied
    bool line_stiffness;
    // lists on the line form whose elements share their factor blocks bit for bit (detect_shared_blocks) read the few
    // distinct blocks instead of streaming every copy; 0: every element streams its own.  The words read are the same, so
    // are all bits
    bool shared_factor_blocks;
    // lists on the line form whose uploaded D_hat has a zero interior diagonal and is its own negated mirror image
    // (check_lean_table) run the lean instance, which leaves out the addition of exact zeros; 0: the parent instances.  The
    // values are the parent's, to the sign of a zero, so nothing that hangs on the operator is emptied
    bool lean_line_stiffness;
    // a Subdomain whose lists all run the degree-7 line form in double has that kernel complete the rows of the gather Qt that
    // have one entry, or two from neighbouring elements of one workgroup, and gathers the other rows alone
    // (assembly_classes.hpp; where Subdomain::assembly_obstacle finds none); 0: the point buffer and the whole
    // gather.  The sums are the gather's own statements, so every bit stays and nothing that hangs on the operator is emptied
    bool assemble_in_stiffness;
    // lists on the line form that carry a coefficient (LevelList::coef: a diffusivity on a list whose unscaled factor
    // blocks repeat) run the coefficient instance, which reads the shared unscaled block and one coefficient per point and
    // forms the scaled factor itself; 0: they stream the scaled arrays.  The product is the statement that made the scaled
    // arrays, so the bits are the streamed instance's and nothing that hangs on the operator is emptied.  On by default where
    // its entries are, like the flags above (measured faster than streaming the scaled arrays); the
    // initialiser is what a kernel library without the entries leaves
    bool coefficient_in_kernel = false;

    StiffnessFlags();
};

// flag name -> member and the entries it needs, in the order in which a missing one is named
struct StiffnessFlagRow
{
    const char *name;
    bool StiffnessFlags::*member;
    struct
    {
        const void *fn;
        const char *name;
    } entries[5]; // ends at a null name
};

inline const std::array<StiffnessFlagRow, 8> &stiffness_flag_table()
{
#define FDD_ENTRY(name) {(const void *)&name, #name}
    static const std::array<StiffnessFlagRow, 8> table = {{
        {"mfma_stiffness", &StiffnessFlags::mfma_stiffness, {}},
        {"skip_zero_factors", &StiffnessFlags::skip_zero_factors, {FDD_ENTRY(fdd_stiffness_offdiag_zero), FDD_ENTRY(fdd_stiffness_matrix_diag), FDD_ENTRY(fdd_stiffness_matrix_diag_f32)}},
        // with the check that sets LevelList::offdiag_zero
        {"mfma_skip_zero_factors", &StiffnessFlags::mfma_skip_zero_factors, {FDD_ENTRY(fdd_stiffness_matrix_mfma_diag), FDD_ENTRY(fdd_stiffness_offdiag_zero), FDD_ENTRY(fdd_stiffness_matrix_diag), FDD_ENTRY(fdd_stiffness_matrix_diag_f32)}},
        {"line_stiffness", &StiffnessFlags::line_stiffness, {FDD_ENTRY(fdd_stiffness_matrix_lines), FDD_ENTRY(fdd_stiffness_matrix_lines_f32)}},
        // with the two entries that establish which blocks repeat
        {"shared_factor_blocks", &StiffnessFlags::shared_factor_blocks, {FDD_ENTRY(fdd_stiffness_matrix_lines_shared), FDD_ENTRY(fdd_stiffness_matrix_lines_shared_f32), FDD_ENTRY(fdd_stiffness_factor_block_hash), FDD_ENTRY(fdd_stiffness_factor_block_verify)}},
        {"lean_line_stiffness", &StiffnessFlags::lean_line_stiffness, {FDD_ENTRY(fdd_stiffness_matrix_lines_lean), FDD_ENTRY(fdd_stiffness_matrix_lines_lean_f32)}},
        // with the gather of the rows the kernel leaves
        {"assemble_in_stiffness", &StiffnessFlags::assemble_in_stiffness, {FDD_ENTRY(fdd_stiffness_matrix_lines_direct), FDD_ENTRY(fdd_csr_plan_gather_mapped)}},
        {"coefficient_in_kernel", &StiffnessFlags::coefficient_in_kernel, {FDD_ENTRY(fdd_stiffness_matrix_lines_coef), FDD_ENTRY(fdd_stiffness_matrix_lines_coef_f32), FDD_ENTRY(fdd_stiffness_matrix_lines_coef_direct)}},
    }};
#undef FDD_ENTRY
    return table;
}

inline const StiffnessFlagRow *stiffness_flag_row(const std::string &flag)
{
    for (const StiffnessFlagRow &row : stiffness_flag_table())
        if (flag == row.name) return &row;
    return nullptr;
}

// the first entry the flag needs that the loaded kernel library does not export, or nullptr
inline const char *missing_stiffness_entry(const StiffnessFlagRow &row)
{
    for (const auto &e : row.entries)
        if (e.name and e.fn == nullptr) return e.name;
    return nullptr;
}
inline const char *missing_stiffness_entry(const char *flag) { return missing_stiffness_entry(*stiffness_flag_row(flag)); }

inline StiffnessFlags::StiffnessFlags()
{
    for (const StiffnessFlagRow &row : stiffness_flag_table()) this->*row.member = missing_stiffness_entry(row) == nullptr;
}

// false: not a stiffness flag.  Throws where the flag is to be turned on and an entry it needs is missing
inline bool set_stiffness_flag(StiffnessFlags &flags, const std::string &flag, bool on)
{
    const StiffnessFlagRow *row = stiffness_flag_row(flag);
    if (not row) return false;
    if (on)
        if (const char *missing = missing_stiffness_entry(*row)) throw std::runtime_error(flag + " needs " + missing + ", which the loaded kernel library does not export");
    flags.*row->member = on;
    return true;
}
inline bool stiffness_flag(const StiffnessFlags &flags, const char *flag) { return flags.*stiffness_flag_row(flag)->member; }

// ---- factor arrays that are identically zero (flag "skip_zero_factors") ----
// On a mesh whose elements have orthogonal axes (every box, every rectilinear grid) G[3..5] are 0.0 at every point.
// detect_zero_factors establishes that from the list's OWN arrays in one pass on the device; where it holds (and the flag
// is on) the list runs the kernel that streams G[0..2] only.  Unlike the affine option the arithmetic left out is the
// addition of exact zeros: the operator's values are the same, to the sign of a zero.  Only 3-D lists of degree <= 15 are
// checked (the 2-D and two-launch forms keep six arrays); without the entries nothing is, and nothing switches.  A list that
// runs on the matrix cores takes their three-array instance (flag "mfma_skip_zero_factors").
inline void detect_zero_factors(LevelList &ll)
{
    ll.offdiag_zero = false;
    if (ll.dim != 3 or ll.poly_degree > 15 or ll.num_elements == 0 or missing_stiffness_entry("skip_zero_factors")) return;
    int flags[3] = {1, 1, 1};
    memory flags_dev = dev().malloc<int>(3);
    FDD_CALL(fdd_stiffness_offdiag_zero(flags_dev.as<int>(), ll.G, nullptr, ll.num_elements, ll.poly_degree, dev().stream));
    flags_dev.copyTo(flags, sizeof(flags));
    ll.offdiag_zero = flags[0] == 0 and flags[1] == 0 and flags[2] == 0;
}

// ---- factor blocks that repeat from element to element (flag "shared_factor_blocks") ----
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
    ll.factor_elem = memory();
    if (not ll.offdiag_zero or ll.dim != 3 or ll.poly_degree > 15 or ll.num_elements == 0 or missing_stiffness_entry("shared_factor_blocks")) return;
    const size_t ne = (size_t)ll.num_elements;
    std::vector<unsigned long long> hash(ne);
    memory hash_dev = dev().malloc<unsigned long long>(ne);
    FDD_CALL(fdd_stiffness_factor_block_hash(hash_dev.as<unsigned long long>(), ll.G, nullptr, ll.num_elements, ll.poly_degree, dev().stream));
    hash_dev.copyTo(hash.data(), ne * sizeof(unsigned long long));
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
    if (mismatches != 0) return;
    ll.factor_elem = rep_dev;
    ll.shared_blocks = true;
}

// ---- the lean instances of the line form (flag "lean_line_stiffness") ----
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
// (Subdomain::prepare_single_precision) and again when the table changes under it (Subdomain::operator_changed): the verdict
// on it is made wherever the cast is.
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

// ---- which kernel a list runs ----
enum class StiffnessForm
{
    local, // Au = A_L u on element-local points (apply_local; double only)
    gather // q = A_L (Q (s v)), Q read through an index array (apply_gather; 3-D lists of degree <= 15)
};

enum class StiffnessFamily
{
    two_launch, // the reference's two-launch form, degree above 15
    fused_2d,
    fused,      // six factor arrays
    diag,       // three factor arrays, slab form
    lines,      // three factor arrays, line form (degree 7); the only family with the attributes shared and lean
    mfma,       // six arrays on the matrix cores
    mfma_diag,  // three arrays on the matrix cores
    affine,
    mfma_affine
};

struct StiffnessChoice
{
    StiffnessFamily family;
    bool shared = false, lean = false;
    bool coef = false; // the coefficient instance of the line form; never together with shared (it names the blocks itself)

    // what fddh_problem_*_info counts, asked of the gather form's choice
    bool three_arrays() const { return family == StiffnessFamily::diag or family == StiffnessFamily::lines; } // not the matrix-core instance
    bool mfma_three_arrays() const { return family == StiffnessFamily::mfma_diag; }
    bool lines() const { return family == StiffnessFamily::lines; }
    bool shared_lines() const { return lines() and shared; }
    bool lean_lines() const { return lines() and lean; }
    bool coef_lines() const { return lines() and coef; }
};

// The one decision, for both forms and both precisions.  in_place: Au == u (local form only).  Launches nothing, touches no
// device memory and asks no weak symbol (StiffnessFlags); a handful of comparisons, made again at every launch.
inline StiffnessChoice choose_stiffness(const LevelList &ll, const StiffnessFlags &flags, bool f32, StiffnessForm form, bool in_place = false)
{
    using F = StiffnessFamily;
    const bool gather = form == StiffnessForm::gather;
    // the matrix-core kernels exist in double only, for 3-D elements of degree 11..15: a float list never runs on them
    const bool matrix_cores = not f32 and flags.mfma_stiffness and ll.dim == 3 and ll.poly_degree >= 11 and ll.poly_degree <= 15;
    // the gather form takes affine first, whatever the other flags say
    if (gather and ll.affine) return {matrix_cores ? F::mfma_affine : F::affine};
    // the local form has no affine kernel: an affine list there runs six arrays
    const bool three_arrays = flags.skip_zero_factors and ll.offdiag_zero and not ll.affine;
    // the local matrix-core kernels need Au != u; in place, such a list runs six arrays off the matrix cores
    if (matrix_cores and (gather or not in_place)) return {three_arrays and flags.mfma_skip_zero_factors ? F::mfma_diag : F::mfma};
    if (three_arrays and not matrix_cores)
    {
        if (not(flags.line_stiffness and ll.dim == 3 and ll.poly_degree == 7)) return {F::diag};
        // shared or streamed, a lean list or not: the two attributes do not look at each other, and each precision's lean
        // verdict comes from the check of its own table
        const bool lean = flags.lean_line_stiffness and (f32 ? ll.lean_D_hat32 : ll.lean_D_hat);
        // a list that carries a coefficient, while the flag is on: the coefficient instance (its entries refuse Au == u)
        if (ll.coef.ptr() and flags.coefficient_in_kernel and not in_place) return {F::lines, false, lean, true};
        return {F::lines, flags.shared_factor_blocks and ll.shared_blocks, lean};
    }
    if (gather or (ll.dim == 3 and ll.poly_degree <= 15)) return {F::fused};
    return {ll.dim == 2 and ll.poly_degree <= 15 ? F::fused_2d : F::two_launch};
}

// The profile label and the bytes per point of every choice: the strings and numbers bench.py's kernel table keys on.  The
// labels of the three-array instances are not "fused_stiffness_kernel..." / "mfma_stiffness_kernel...": the committed counters
// bench.py matches by those prefixes are the six-array kernels'.  The line form counts the bytes of the instance it replaces
// (lean: of its parent instance); a shared list's few factor blocks stay in cache, so u and Au (index and q) are what moves.
// The gather form adds the gathered values to its total (apply_gather).  No label: no scope (the two-launch form).
struct StiffnessProfile
{
    const char *label;
    double bytes_per_point;
};
inline StiffnessProfile stiffness_profile(StiffnessForm form, const StiffnessChoice &c, bool f32)
{
    using F = StiffnessFamily;
    static const struct
    {
        StiffnessForm form;
        F family;
        bool shared, lean, coef;
        const char *label, *label32;
        double bytes, bytes32;
    } table[] = {
        {StiffnessForm::local, F::mfma_diag, false, false, false, "mfma_diag_stiffness_kernel", nullptr, 40.0, 0.0},
        {StiffnessForm::local, F::mfma, false, false, false, "mfma_stiffness_kernel", nullptr, 64.0, 0.0},
        {StiffnessForm::local, F::lines, false, false, false, "line_stiffness_kernel", nullptr, 40.0, 0.0},
        {StiffnessForm::local, F::lines, true, false, false, "line_stiffness_kernel<shared>", nullptr, 16.0, 0.0},
        {StiffnessForm::local, F::lines, false, true, false, "line_stiffness_kernel<lean>", nullptr, 40.0, 0.0},
        {StiffnessForm::local, F::lines, true, true, false, "line_stiffness_kernel<shared,lean>", nullptr, 16.0, 0.0},
        // the coefficient instances: the shared instance's bytes plus one double per point for the coefficient, in both
        // precisions (its second and third read per element are expected to come from cache: derived)
        {StiffnessForm::local, F::lines, false, false, true, "line_stiffness_kernel<coef>", nullptr, 24.0, 0.0},
        {StiffnessForm::local, F::lines, false, true, true, "line_stiffness_kernel<coef,lean>", nullptr, 24.0, 0.0},
        {StiffnessForm::local, F::diag, false, false, false, "diag_stiffness_kernel", nullptr, 40.0, 0.0},
        {StiffnessForm::local, F::fused, false, false, false, "fused_stiffness_kernel", nullptr, 64.0, 0.0},
        {StiffnessForm::local, F::fused_2d, false, false, false, "fused_stiffness_2d_kernel", nullptr, 40.0, 0.0},
        {StiffnessForm::gather, F::affine, false, false, false, "fused_stiffness_kernel<gather,affine>", "fused_stiffness_kernel<gather,f32,affine>", 12.0, 8.0},
        {StiffnessForm::gather, F::mfma_affine, false, false, false, "mfma_stiffness_kernel<gather,affine>", nullptr, 12.0, 0.0},
        {StiffnessForm::gather, F::mfma_diag, false, false, false, "mfma_diag_stiffness_kernel<gather>", nullptr, 36.0, 0.0},
        {StiffnessForm::gather, F::lines, false, false, false, "line_stiffness_kernel<gather>", "line_stiffness_kernel<gather,f32>", 36.0, 20.0},
        {StiffnessForm::gather, F::lines, true, false, false, "line_stiffness_kernel<gather,shared>", "line_stiffness_kernel<gather,shared,f32>", 12.0, 8.0},
        {StiffnessForm::gather, F::lines, false, true, false, "line_stiffness_kernel<gather,lean>", "line_stiffness_kernel<gather,f32,lean>", 36.0, 20.0},
        {StiffnessForm::gather, F::lines, true, true, false, "line_stiffness_kernel<gather,shared,lean>", "line_stiffness_kernel<gather,shared,f32,lean>", 12.0, 8.0},
        {StiffnessForm::gather, F::lines, false, false, true, "line_stiffness_kernel<gather,coef>", "line_stiffness_kernel<gather,coef,f32>", 20.0, 16.0},
        {StiffnessForm::gather, F::lines, false, true, true, "line_stiffness_kernel<gather,coef,lean>", "line_stiffness_kernel<gather,coef,f32,lean>", 20.0, 16.0},
        {StiffnessForm::gather, F::diag, false, false, false, "diag_stiffness_kernel<gather>", "diag_stiffness_kernel<gather,f32>", 36.0, 20.0},
        {StiffnessForm::gather, F::fused, false, false, false, "fused_stiffness_kernel<gather>", "fused_stiffness_kernel<gather,f32>", 60.0, 32.0},
        {StiffnessForm::gather, F::mfma, false, false, false, "mfma_stiffness_kernel<gather>", nullptr, 60.0, 0.0},
    };
    for (const auto &row : table)
        if (row.form == form and row.family == c.family and row.shared == c.shared and row.lean == c.lean and row.coef == c.coef) return {f32 ? row.label32 : row.label, f32 ? row.bytes32 : row.bytes};
    return {nullptr, 0.0};
}

// Where a list's arrays come from, by precision: the list's own in double, the float copies in single
template <typename Real>
struct ListArrays
{
    const Real *G[NUM_GEOM_FACTS], *D_hat, *affine_c, *affine_w;
    explicit ListArrays(const LevelList &ll)
    {
        if constexpr (std::is_same<Real, float>::value)
        {
            for (int g = 0; g < NUM_GEOM_FACTS; g++) G[g] = ll.G32[g].as<float>();
            D_hat = ll.D_hat32.as<float>(), affine_c = ll.affine_c32.as<float>(), affine_w = ll.affine_w32.as<float>();
        }
        else
        {
            for (int g = 0; g < NUM_GEOM_FACTS; g++) G[g] = ll.G[g];
            D_hat = ll.D_hat, affine_c = ll.affine_c.as<double>(), affine_w = ll.affine_w.as<double>();
        }
    }
};

// the arguments of the coefficient entries that come from the list: double in both precisions
struct CoefArrays
{
    const double *coef, *blocks[3];
    const int *block_of_elem;
    explicit CoefArrays(const LevelList &ll) : coef(ll.coef.as<double>()), blocks{ll.coef_blocks[0].as<double>(), ll.coef_blocks[1].as<double>(), ll.coef_blocks[2].as<double>()}, block_of_elem(ll.coef_block_of_elem.as<int>()) {}
};

// an entry of the kernel library by precision
template <typename Real, typename Entry64, typename Entry32>
inline auto entry_of(Entry64 *entry, Entry32 *entry_f32)
{
    if constexpr (std::is_same<Real, float>::value)
        return entry_f32;
    else
        return entry;
}

// the families on three factor arrays take the same arguments in both forms (local: no index, no scale).  False: not one of them
template <typename Real>
inline bool launch_three_arrays(const StiffnessChoice &c, const LevelList &ll, Real *q, const Real *v, const double *scale_dev, const int *point_index)
{
    const ListArrays<Real> a(ll);
    void *s = dev().stream;
    const int *factor_elem = c.shared ? ll.factor_elem.as<int>() : nullptr;
    if (c.family == StiffnessFamily::diag)
        FDD_CALL(entry_of<Real>(fdd_stiffness_matrix_diag, fdd_stiffness_matrix_diag_f32)(q, v, scale_dev, point_index, a.D_hat, a.G, nullptr, ll.num_elements, ll.poly_degree, s));
    else if (c.family == StiffnessFamily::mfma_diag)
    {
        if constexpr (std::is_same<Real, double>::value) FDD_CALL(fdd_stiffness_matrix_mfma_diag(q, v, scale_dev, point_index, a.D_hat, a.G, nullptr, ll.num_elements, ll.poly_degree, s));
    }
    else if (c.family != StiffnessFamily::lines)
        return false;
    else if (c.coef) // the table is the precision's own
    {
        const CoefArrays k(ll);
        FDD_CALL(entry_of<Real>(fdd_stiffness_matrix_lines_coef, fdd_stiffness_matrix_lines_coef_f32)(q, v, scale_dev, point_index, a.D_hat, k.coef, k.blocks, k.block_of_elem, nullptr, c.lean ? 1 : 0, ll.num_elements, ll.poly_degree, 1, s));
    }
    else if (c.lean) // shared where factor_elem is given
        FDD_CALL(entry_of<Real>(fdd_stiffness_matrix_lines_lean, fdd_stiffness_matrix_lines_lean_f32)(q, v, scale_dev, point_index, a.D_hat, a.G, nullptr, factor_elem, ll.num_elements, ll.poly_degree, 1, s));
    else if (c.shared)
        FDD_CALL(entry_of<Real>(fdd_stiffness_matrix_lines_shared, fdd_stiffness_matrix_lines_shared_f32)(q, v, scale_dev, point_index, a.D_hat, a.G, nullptr, factor_elem, ll.num_elements, ll.poly_degree, 1, s));
    else
        FDD_CALL(entry_of<Real>(fdd_stiffness_matrix_lines, fdd_stiffness_matrix_lines_f32)(q, v, scale_dev, point_index, a.D_hat, a.G, nullptr, ll.num_elements, ll.poly_degree, 1, s));
    return true;
}

// Au = A_L u on the points of the list (Au, u: the vectors the list's first_offset counts in).  workspace: three vectors
// of the list's points for the two-launch form above degree 15.
inline void apply_local(const LevelList &ll, double *Au, const double *u, const std::vector<memory> &workspace, const StiffnessFlags &flags)
{
    void *stream = dev().stream;
    Au += ll.first_offset, u += ll.first_offset;
    const StiffnessChoice c = choose_stiffness(ll, flags, false, StiffnessForm::local, Au == u);
    if (c.family == StiffnessFamily::two_launch)
    {
        // degree above 15: the reference's two-launch form (domain.tpp:605-606) on the list
        double *GDu[3] = {workspace[0].as<double>(), workspace[1].as<double>(), workspace[2].as<double>()};
        FDD_CALL(fdd_dom_stiffness_matrix_1(GDu, u, ll.D_hat, ll.G, (int)ll.num_points(), ll.poly_degree, ll.dim, stream));
        FDD_CALL(fdd_dom_stiffness_matrix_2(Au, GDu, ll.D_hat, (int)ll.num_points(), ll.poly_degree, ll.dim, stream));
        return;
    }
    const StiffnessProfile p = stiffness_profile(StiffnessForm::local, c, false);
    ProfileScope prof(p.label, p.bytes_per_point * (double)ll.num_points());
    if (launch_three_arrays<double>(c, ll, Au, u, nullptr, nullptr)) return;
    if (c.family == StiffnessFamily::mfma) // high order: the six contractions on the fp64 matrix cores (tolerance-level parity, fdd_hip.h)
        FDD_CALL(fdd_stiffness_matrix_mfma(Au, u, ll.D_hat, ll.G, nullptr, ll.num_elements, ll.poly_degree, stream));
    else if (c.family == StiffnessFamily::fused)
        FDD_CALL(fdd_sub_stiffness_matrix(Au, u, ll.D_hat, ll.G, nullptr, ll.num_elements, ll.poly_degree, stream));
    else
        FDD_CALL(fdd_stiffness_matrix_2d(Au, u, ll.D_hat, ll.G, nullptr, ll.num_elements, ll.poly_degree, stream));
}

// q (points of the list) = A_L (Q (s v)): u[p] = s v[point_index[p]] on load (0 where the index is negative), s = *scale_dev
// (null: 1).  q, point_index: the arrays the list's first_offset counts in; gathered_values: the length of v (the bytes it
// adds to the count).  3-D lists of degree <= 15.
template <typename Real>
inline void apply_gather(const LevelList &ll, Real *q, const Real *v, const int *point_index, const double *scale_dev, int gathered_values, const StiffnessFlags &flags)
{
    constexpr bool f32 = std::is_same<Real, float>::value;
    void *stream = dev().stream;
    q += ll.first_offset, point_index += ll.first_offset;
    const StiffnessChoice c = choose_stiffness(ll, flags, f32, StiffnessForm::gather);
    const StiffnessProfile p = stiffness_profile(StiffnessForm::gather, c, f32);
    ProfileScope prof(p.label, p.bytes_per_point * (double)ll.num_points() + (double)sizeof(Real) * gathered_values);
    if (launch_three_arrays<Real>(c, ll, q, v, scale_dev, point_index)) return;
    const ListArrays<Real> a(ll);
    const bool matrix_cores = c.family == StiffnessFamily::mfma or c.family == StiffnessFamily::mfma_affine; // never in float (choose_stiffness)
    if (c.family == StiffnessFamily::affine or c.family == StiffnessFamily::mfma_affine)
    {
        if constexpr (f32)
            FDD_CALL(fdd_stiffness_matrix_affine_f32(q, v, scale_dev, point_index, a.D_hat, a.affine_c, a.affine_w, nullptr, ll.num_elements, ll.poly_degree, stream));
        else
            FDD_CALL((matrix_cores ? fdd_stiffness_matrix_mfma_affine : fdd_stiffness_matrix_affine)(q, v, scale_dev, point_index, a.D_hat, a.affine_c, a.affine_w, nullptr, ll.num_elements, ll.poly_degree, stream));
    }
    else if constexpr (f32)
        FDD_CALL(fdd_sub_stiffness_matrix_gather_scaled_f32(q, v, scale_dev, point_index, a.D_hat, a.G, nullptr, ll.num_elements, ll.poly_degree, stream));
    else
        FDD_CALL((matrix_cores ? fdd_stiffness_matrix_mfma_gather : fdd_sub_stiffness_matrix_gather_scaled)(q, v, scale_dev, point_index, a.D_hat, a.G, nullptr, ll.num_elements, ll.poly_degree, stream));
}

// ---- the line form that assembles (flag "assemble_in_stiffness") ----
// Can the list run it?  The gather form's choice in double is the line form, whichever instance
inline bool direct_lines_apply(const LevelList &ll, const StiffnessFlags &flags) { return flags.assemble_in_stiffness and choose_stiffness(ll, flags, false, StiffnessForm::gather).lines(); }

// apply_gather with the rows of y = Qt q that the kernel completes written to y and the other points' values to q;
// point_class_dof: point_index with the class of every point (assembly_classes.hpp).  The caller has asked direct_lines_apply.
// The instance is the one choose_stiffness names and the launch is recorded under that instance's label, with its count:
// every point's value is still stored once, or handed to the neighbour's store.  What tells the two paths apart in a profile
// is the gather that follows (AssemblyClasses::gather_general)
inline void apply_gather_direct(const LevelList &ll, double *q, double *y, const double *v, const int *point_class_dof, const double *scale_dev, int gathered_values, const StiffnessFlags &flags)
{
    q += ll.first_offset, point_class_dof += ll.first_offset;
    const StiffnessChoice c = choose_stiffness(ll, flags, false, StiffnessForm::gather);
    const StiffnessProfile p = stiffness_profile(StiffnessForm::gather, c, false);
    ProfileScope prof(p.label, p.bytes_per_point * (double)ll.num_points() + (double)sizeof(double) * gathered_values);
    if (c.coef)
    {
        const CoefArrays k(ll);
        FDD_CALL(fdd_stiffness_matrix_lines_coef_direct(q, y, v, scale_dev, point_class_dof, ll.D_hat, k.coef, k.blocks, k.block_of_elem, nullptr, c.lean ? 1 : 0, ll.num_elements, ll.poly_degree, 1, dev().stream));
        return;
    }
    FDD_CALL(fdd_stiffness_matrix_lines_direct(q, y, v, scale_dev, point_class_dof, ll.D_hat, ll.G, nullptr, c.shared ? ll.factor_elem.as<int>() : nullptr, c.lean ? 1 : 0, ll.num_elements, ll.poly_degree, 1, dev().stream));
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
