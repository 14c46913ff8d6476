/*
 * diffusivity.hpp -- a diffusivity per point: -div(kappa grad u) on the lists of element_operator.hpp -- a LABELLED OPTION of
 * this build (the reference solves the Poisson problem).
 *
 * kappa_p is one double per point of the fine level, element-major like the mesh's coordinates, finite and > 0; continuity
 * across elements is not asked for.  The local operator becomes A_L u = D^T [kappa G] D u, and the whole of it is a second set
 * of factor arrays
 *
 *     G'[g][p] = mesh.g[g][p] * kappa[p]        one IEEE double product per entry, on the host, for all six g
 *
 * uploaded into the buffers the lists already point to: every stiffness kernel, the exact Jacobi diagonal and whatever else
 * reads a list's arrays follows without knowing.  A zero stays a zero, so the three-array kernels keep applying.  The mesh's
 * own arrays are never written: setting again or clearing starts from them.
 *
 * What this file holds: the checks of a caller's kappa, the product, what has to be derived again from a list's arrays once
 * they change (refresh_list), and the members of the coefficient line instance (LevelList::coef...), which reads the
 * unscaled blocks of a list whose blocks repeat and forms the product itself.  Domain::set_diffusivity and
 * Subdomain::set_diffusivity call it; the low-order hierarchy takes kappa through low_order::assemble_fem.
 */
#ifndef FDD_DIFFUSIVITY_HPP
#define FDD_DIFFUSIVITY_HPP

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "element_operator.hpp"

namespace fdd
{
namespace diffusivity
{

// a refusal's text with its numbers in it
template <typename... Args>
inline std::string formatted(const char *format, Args... args)
{
    char msg[256];
    snprintf(msg, sizeof(msg), format, args...);
    return msg;
}

// Why a kappa of n values cannot be set on a problem of num_points fine-level points, or "": nothing is touched before this
// has passed.  The first offending point is named.
inline std::string refusal(const double *kappa, long long n, long long num_points, int dim, int ranks, bool composite)
{
    if (ranks > 1) return formatted("a diffusivity is supported on one rank: this communicator has %d", ranks);
    if (composite) return "a diffusivity needs a conforming region: this problem's Subdomain is a composite (its rings would need the neighbours' kappa at reduced degree)";
    if (dim != 3) return formatted("a diffusivity is 3-D only: this problem is %d-D", dim);
    if (kappa == nullptr) return "";
    if (n != num_points) return formatted("kappa has one value per point of the fine level (%lld), got %lld", num_points, n);
    for (long long p = 0; p < n; p++)
        if (not std::isfinite(kappa[p]) or not(kappa[p] > 0.0)) return formatted("kappa must be finite and > 0 at every point: point %lld has %g", p, kappa[p]);
    return "";
}

// G'[p] = g[p] * kappa[p] (kappa == nullptr: the mesh's own values) into the device buffer a list reads
inline void upload_scaled(memory &dst, const std::vector<double> &g, const double *kappa)
{
    if (kappa == nullptr)
    {
        dst.copyFrom(g.data(), g.size() * sizeof(double));
        return;
    }
    std::vector<double> scaled(g.size());
    for (size_t p = 0; p < g.size(); p++) scaled[p] = g[p] * kappa[p];
    dst.copyFrom(scaled.data(), scaled.size() * sizeof(double));
}

// What detect_shared_blocks found on a list's UNSCALED arrays, kept from before the first kappa is uploaded: the scaled
// blocks of a variable kappa do not repeat, the unscaled ones still do, and the coefficient instance reads those
struct UnscaledBlocks
{
    bool known = false, shared = false;
    std::vector<int> factor_elem;

    // call while the list's arrays are still the mesh's own
    void remember(const LevelList &ll)
    {
        if (known) return;
        known = true;
        shared = ll.shared_blocks;
        factor_elem.resize(shared ? (size_t)ll.num_elements : 0);
        if (shared) ll.factor_elem.copyTo(factor_elem.data(), factor_elem.size() * sizeof(int));
    }
};

inline void clear_coef(LevelList &ll)
{
    ll.coef = ll.coef_block_of_elem = memory();
    for (memory &m : ll.coef_blocks) m = memory();
}

// The members of the coefficient instance, for a 3-D degree-7 list whose unscaled arrays share blocks: kappa on the
// device, the distinct unscaled blocks of g[0..2] (host arrays over the list's points) one after another in ascending order
// of the element that holds them, and every element's block.  Nothing where the list is another
inline void fill_coef(LevelList &ll, const UnscaledBlocks &ub, const double *kappa, const std::vector<double> *const g[3])
{
    clear_coef(ll);
    if (kappa == nullptr or not ub.shared or ll.dim != 3 or ll.poly_degree != 7 or ll.num_elements == 0) return;
    const size_t ne = (size_t)ll.num_elements, n3 = 512, base = (size_t)ll.first_offset;
    std::vector<int> reps(ub.factor_elem);
    std::sort(reps.begin(), reps.end());
    reps.erase(std::unique(reps.begin(), reps.end()), reps.end());
    std::vector<int> block_of_elem(ne);
    for (size_t e = 0; e < ne; e++) block_of_elem[e] = (int)(std::lower_bound(reps.begin(), reps.end(), ub.factor_elem[e]) - reps.begin());
    std::vector<double> compact(reps.size() * n3);
    for (int f = 0; f < 3; f++)
    {
        for (size_t c = 0; c < reps.size(); c++) std::copy_n(g[f]->data() + base + (size_t)reps[c] * n3, n3, compact.data() + c * n3);
        ll.coef_blocks[f] = dev().malloc<double>(compact.size());
        ll.coef_blocks[f].copyFrom(compact.data(), compact.size() * sizeof(double));
    }
    ll.coef_block_of_elem = dev().malloc<int>(ne);
    ll.coef_block_of_elem.copyFrom(block_of_elem.data(), ne * sizeof(int));
    ll.coef = dev().malloc<double>(ne * n3);
    ll.coef.copyFrom(kappa + base, ne * n3 * sizeof(double));
}

// the same members as views of another list's over the same elements (the Subdomain's level-0 list on the Domain's): not owned
inline void share_coef(LevelList &ll, const LevelList &owner)
{
    clear_coef(ll);
    if (not owner.coef.ptr()) return;
    ll.coef = owner.coef.slice(0, owner.coef.size());
    for (int f = 0; f < 3; f++) ll.coef_blocks[f] = owner.coef_blocks[f].slice(0, owner.coef_blocks[f].size());
    ll.coef_block_of_elem = owner.coef_block_of_elem.slice(0, owner.coef_block_of_elem.size());
}

// The arrays behind ll.G have been rewritten in place: everything derived from them is derived again -- are the
// off-diagonal arrays zero, do blocks repeat, are the elements affine (only where that option was asked for), and the float
// copies where they exist.  D_hat has not changed, so the lean verdicts stay
inline void refresh_list(LevelList &ll)
{
    detect_zero_factors(ll);
    detect_shared_blocks(ll);
    const bool had_float_affine = ll.affine_c32.ptr() != nullptr;
    ll.affine_deviation = -1.0;
    ll.affine_c = ll.affine_w = ll.affine_c32 = ll.affine_w32 = memory();
    ll.affine = ll.affine_requested and detect_affine(ll);
    if (had_float_affine) affine_float_copies(ll);
    const size_t np = ll.num_points();
    for (int g = 0; g < NUM_GEOM_FACTS; g++)
        if (ll.G32[g].ptr()) FDD_CALL(fdd_sub_copy_f32_f64(ll.G32[g].as<float>(), ll.G[g], (int)np, dev().stream));
}

} // namespace diffusivity
} // namespace fdd

#endif
