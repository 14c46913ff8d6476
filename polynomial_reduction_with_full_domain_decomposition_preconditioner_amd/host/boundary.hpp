/*
 * boundary.hpp -- Neumann and Robin faces of the generated box meshes -- a LABELLED OPTION of this build (every problem of
 * the reference is homogeneous Dirichlet through the mask its mesh files carry), the counterpart of helmholtz.hpp.
 *
 * The faces of the cube are x-, x+, y-, y+, z-, z+ (side s = 2 axis + upper); BoxSpec::faces says which are Dirichlet ('D',
 * masked) and which natural ('N', unknowns).  On a natural face the weak form leaves the surface integral of the flux, which
 * the caller adds to the right-hand side (Neumann data), and a Robin condition kappa du/dn + alpha u = g adds
 *
 *     r[q] = sum over the face entries (f, a, b) at point q of alpha(f, a, b) * area(f, a, b)
 *
 * to the diagonal: the surface mass matrix of the GLL points is diagonal like the volume one.  r joins the Helmholtz
 * products lambda_q B_q per point, and everything behind Domain::set_shift follows (fdd_host_capi.cpp: rebuild_shift).
 *
 * What this file holds: the checks of face codes and of a caller's alpha, the face list of a generated mesh, the index of a
 * face point in a point vector, the sums r, and the compressed form of a shift that is zero on most of its vector.
 */
#ifndef FDD_BOUNDARY_HPP
#define FDD_BOUNDARY_HPP

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "box_mesh.hpp"
#include "diffusivity.hpp"
#include "fdd_device.hpp"

namespace fdd
{
namespace boundary
{

// A shift whose support is at most 1 / kIndexedShiftShare of its vector runs fdd_shift_add_indexed (flag "indexed_shift").
// Derived, not measured: at worst an entry of the indexed pass moves three 128-byte lines (y, x and, shared with its
// neighbours, c_values / index: 8 + 4 B) -- 3 * 128 + 12 = 396 B -- where the dense pass moves 32 B per dof (y read and
// written, c, x).  396 / 32 = 12.4; the next power of two leaves the indexed pass at most 0.78 of the dense bytes.
constexpr int kIndexedShiftShare = 16;

// why `codes` cannot be face codes, or ""
inline std::string faces_refusal(const char *codes)
{
    using diffusivity::formatted;
    if (codes == nullptr) return "face codes: null argument";
    const size_t len = std::strlen(codes);
    if (len != 6) return formatted("face codes are six characters (x-, x+, y-, y+, z-, z+), got %zu", len);
    for (int s = 0; s < 6; s++)
        if (codes[s] != 'D' and codes[s] != 'N') return formatted("face code %d is '%c': 'D' (Dirichlet) or 'N' (natural)", s, codes[s]);
    return "";
}

// every face of the rank's elements that lies on the surface of the box, sorted by (side, element)
struct FaceList
{
    std::vector<int> elem, side;
    int size() const { return (int)elem.size(); }
};

inline FaceList box_faces(const BoxSpec &spec, int rank)
{
    FaceList list;
    int l[3], o[3];
    const int r[3] = {rank % spec.P[0], (rank / spec.P[0]) % spec.P[1], rank / (spec.P[0] * spec.P[1])};
    for (int d = 0; d < 3; d++)
    {
        l[d] = spec.E[d] / spec.P[d];
        o[d] = r[d] * l[d];
    }
    for (int s = 0; s < 6; s++)
    {
        const int axis = s >> 1, want = (s & 1) ? spec.E[axis] - 1 : 0;
        for (int e = 0; e < l[0] * l[1] * l[2]; e++)
        {
            const int ex[3] = {e % l[0], (e / l[0]) % l[1], e / (l[0] * l[1])};
            if (o[axis] + ex[axis] != want) continue;
            list.elem.push_back(e);
            list.side.push_back(s);
        }
    }
    return list;
}

// the index in a point vector of face point (a, b) of side s of element e: (a, b) = (j, k) on r-faces, (i, k) on s-faces,
// (i, j) on t-faces (include/fdd_hip.h: fdd_field_surface)
inline long long face_point(int e, int s, int a, int b, int n)
{
    const int axis = s >> 1, fixed = (s & 1) ? n - 1 : 0;
    const long long in_elem = axis == 0 ? fixed + (long long)n * (a + n * b) : (axis == 1 ? a + (long long)n * (fixed + n * b) : a + (long long)n * (b + n * fixed));
    return (long long)e * n * n * n + in_elem;
}

// why alpha (one value per face point, faces.size() n^2 of them) cannot be set, or "": finite and >= 0, and 0 on every
// point the mask holds at zero (a point of a 'D' face: the value there is prescribed, a Robin term would never be seen)
template <typename Mask>
std::string robin_refusal(const double *alpha, const FaceList &faces, int n, const Mask &p_mask)
{
    using diffusivity::formatted;
    for (int f = 0; f < faces.size(); f++)
        for (int ab = 0; ab < n * n; ab++)
        {
            const double v = alpha[(size_t)f * n * n + ab];
            if (not std::isfinite(v) or v < 0.0) return formatted("alpha must be finite and >= 0 at every face point: face %d (element %d, side %d), point %d has %g", f, faces.elem[f], faces.side[f], ab, v);
            if (v > 0.0 and p_mask[(size_t)face_point(faces.elem[f], faces.side[f], ab % n, ab / n, n)] == 0.0)
                return formatted("a Robin coefficient on a Dirichlet point: face %d (element %d, side %d), point %d has alpha = %g and lies on a 'D' face", f, faces.elem[f], faces.side[f], ab, v);
        }
    return "";
}

// r[q] = sum alpha * area over the face entries at point q, in face-list order, from 0.0
inline std::vector<double> robin_points(const double *alpha, const double *area, const FaceList &faces, int n, size_t num_points)
{
    std::vector<double> r(num_points, 0.0);
    for (int f = 0; f < faces.size(); f++)
        for (int ab = 0; ab < n * n; ab++)
        {
            const size_t k = (size_t)f * n * n + ab;
            const size_t q = (size_t)face_point(faces.elem[f], faces.side[f], ab % n, ab / n, n);
            r[q] = r[q] + alpha[k] * area[k];
        }
    return r;
}

// The entries of a shift c that are not zero, compressed: ascending indices, the values in both precisions.  A member of
// Domain (nodes) and of Subdomain (dofs), made where their set_shift stores c.  Only a candidate is compressed: the support
// is counted first, and a c whose support is above 1 / kIndexedShiftShare of it (every Helmholtz shift: lambda B > 0 on all
// nodes), or a kernel library without the entries, allocates and uploads nothing -- no flag setting could make such a c run
// the indexed pass.  count is the support either way.
struct ShiftSupport
{
    memory index, values, values_f32;
    int count = 0;
    bool compressed = false;

    ShiftSupport() {}
    ShiftSupport(const ShiftSupport &) = delete;
    ShiftSupport &operator=(const ShiftSupport &) = delete;

    void release()
    {
        index = values = values_f32 = memory();
        count = 0;
        compressed = false;
    }

    void build(const std::vector<double> &c)
    {
        release();
        long long support = 0;
        for (double v : c) support += v != 0.0;
        count = (int)support;
        if (support == 0 or support * kIndexedShiftShare > (long long)c.size() or missing_indexed_shift_entry() != nullptr) return;
        std::vector<int> idx;
        std::vector<double> val;
        idx.reserve((size_t)support);
        val.reserve((size_t)support);
        for (size_t i = 0; i < c.size(); i++)
            if (c[i] != 0.0)
            {
                idx.push_back((int)i);
                val.push_back(c[i]);
            }
        index = dev().malloc<int>(idx.size());
        index.copyFrom(idx.data(), idx.size() * sizeof(int));
        values = dev().malloc<double>(val.size());
        values.copyFrom(val.data(), val.size() * sizeof(double));
        std::vector<float> val32(val.begin(), val.end()); // the rounding of to_float: the dense pass's float values on the support
        values_f32 = dev().malloc<float>(val32.size());
        values_f32.copyFrom(val32.data(), val32.size() * sizeof(float));
        compressed = true;
    }

    // does a shift over n entries run the indexed pass
    bool applies(bool enabled, long long n) const { return enabled and compressed and (long long)count * kIndexedShiftShare <= n; }
};

} // namespace boundary
} // namespace fdd

#endif
