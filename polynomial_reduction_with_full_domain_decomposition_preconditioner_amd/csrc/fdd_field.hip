// Mass, gradient and weak divergence of fields on the GLL points of a 3-D mesh, gfx950: the two halves the stiffness
// operator is made of, A_L u = D^T [B J^-1 J^-T] D u = wdiv(grad u), as entries of their own, and the diagonal mass
// matrix B = w_i w_j w_k det J.  An option of this build (the reference has no such kernels).
//
// No array holds the metric J^-1: it is formed per point from the coordinates.  J[a][b] = dX_a / dr_b is D_hat applied to
// x, y, z along r, s, t; C = adj J by cofactors, det J = J[0][.] . C[.][0] -- the statements of host/box_mesh.hpp
// (deform_isoparametric) -- and J^-1 = C / det.  Reading x, y, z costs 24 B per point where nine metric arrays would cost 72:
//   mass  32 B/point (24 read,  8 written)   mass    = (w_i w_j) w_k det
//   grad  56 B/point (32 read, 24 written)   grad_a  = (sum_b du/dr_b C[b][a]) / det
//   wdiv  56 B/point (48 read,  8 written)   F_b     = (w_i w_j) w_k sum_a C[b][a] v_a  (= mass sum_a J^-1[b][a] v_a: the
//                                            determinant cancels, so no division), out = D_r^T F_r + D_s^T F_s + D_t^T F_t
// One division per point (grad) or none, not nine: a double division is a dozen instructions, and nine of them would be a
// third of the kernel's arithmetic.  The contractions are written with explicit fused multiply-adds, which
// -ffp-contract=off leaves alone: no reference arithmetic is to be matched bit for bit here (the bar is the long double
// restatement of tests/field_checks.py), a contraction of n terms is n instructions instead of 2n, and the kernels, which
// are bound by arithmetic and LDS reads before they are by memory, need a third fewer registers for it.
//
// The shape is that of fused_stiffness_kernel_t (fdd_stiffness.hip): an element of n = N+1 points per edge is owned by
// n*n lanes, lane (i,j) marches over k.  Its k-columns of the differentiated fields (x, y, z and, for grad, u) sit in
// registers for the t contraction; only the current k-slab of each sits in LDS (rows padded by one double, two buffers: one
// sync per slab) for the r and s contractions.  wdiv's second half is that kernel's: F_r / F_s slabs through LDS, D_t^T F_t
// accumulated in registers.  A column is a vector value, not an array: slab k's entry is taken out of it (and wdiv's r/s
// part put into the accumulator) under the loop's wave-uniform k by indexed register moves, so the slab loop stays rolled
// and nothing goes to scratch.
//
// Further down: the surface weights of listed faces (fdd_field_surface) and the convection term c . grad u, pointwise and
// over-integrated (fdd_field_convect, fdd_field_weak_convect), each with its own account.
#include "fdd_common.h"

namespace
{

constexpr int kBlock = 256;

enum FieldOp
{
    kMass = 0,
    kGrad = 1,
    kWdiv = 2
};

struct Ptrs3
{
    const double *p[3];
};
struct OutPtrs3
{
    double *p[3];
};

template <int n>
struct FieldCfg
{
    static constexpr int nn = n * n;
    static constexpr int epb = (kBlock / nn) > 0 ? (kBlock / nn) : 1; // elements per workgroup
    static constexpr int ld = n + 1;                                  // padded LDS row
    static constexpr int slab = n * ld;
    static constexpr int vl = n <= 2 ? 2 : (n <= 4 ? 4 : (n <= 8 ? 8 : 16)); // entries of a column value
};

template <int VL>
struct ColumnOf
{
    typedef double type __attribute__((ext_vector_type(VL)));
};

// fdd_stiffness.hip's: a wave-level fence where an element never straddles a wavefront, else a barrier that waits on the
// LDS counter only (the loads requested for the next slab stay in flight)
template <bool kWaveLocal>
__device__ __forceinline__ void element_sync()
{
    if (kWaveLocal)
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    else
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// kMass: out.p[0] = mass.  kGrad: out.p[0..2] = grad of in.p[0].  kWdiv: out.p[0] = weak divergence of in.p[0..2].
// w: the n GLL weights (kMass, kWdiv).  Elements are contiguous: element e starts at e * n^3.
template <int n, int kOp>
__global__ __launch_bounds__(kBlock) void field_kernel(OutPtrs3 out, Ptrs3 in, Ptrs3 X, const double *__restrict__ D_hat, const double *__restrict__ w, int num_elements)
{
    using C = FieldCfg<n>;
    using Column = typename ColumnOf<C::vl>::type;
    constexpr int nn = C::nn;
    constexpr int n3 = nn * n;
    constexpr bool kWaveLocal = (64 % nn == 0);
    constexpr bool kDReg = (n <= 8); // the D_hat rows / columns of a lane in registers, else re-read from LDS per slab
    constexpr int nd = kDReg ? n : 1;
    constexpr int nF = (kOp == kGrad) ? 4 : 3; // fields differentiated: x, y, z and u
    constexpr bool kWeights = (kOp != kGrad);

    __shared__ double s_D[n * n];
    __shared__ double s_c[2][nF][C::epb][C::slab];                                                // slab k of every field, two buffers
    __shared__ double s_f[2][kOp == kWdiv ? C::epb : 1][kOp == kWdiv ? C::slab : 1];              // F_r / F_s of the slab

    constexpr bool kWaveIsElement = (nn == 64);
    const int tid = threadIdx.x;
    const int e_loc = kWaveIsElement ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid / nn;
    const int ij = tid - e_loc * nn;
    const int j = ij / n;
    const int i = ij - j * n;
    const int elem = blockIdx.x * C::epb + e_loc;
    const bool active = (e_loc < C::epb) && (elem < num_elements);
    const size_t base = active ? (size_t)elem * n3 : 0;
    const int el = active ? e_loc : 0;
    const int lpos = i + j * C::ld;

    // this lane's k-columns, all requested before D_hat is staged; wdiv: v of slab 0 behind them
    Column col[nF];
#pragma unroll
    for (int f = 0; f < nF; f++) col[f] = (Column)(0.0);
    double vq[3] = {0.0, 0.0, 0.0};
    double wij = 0.0;
    if (active)
    {
#pragma unroll
        for (int f = 0; f < 3; f++)
        {
            const double *cp = X.p[f] + base;
#pragma unroll
            for (int k = 0; k < n; k++) col[f][k] = __builtin_nontemporal_load(cp + (ij + k * nn));
        }
        if constexpr (kOp == kGrad)
        {
            const double *up = in.p[0] + base;
#pragma unroll
            for (int k = 0; k < n; k++) col[3][k] = __builtin_nontemporal_load(up + (ij + k * nn));
        }
        if constexpr (kOp == kWdiv)
        {
#pragma unroll
            for (int a = 0; a < 3; a++) vq[a] = __builtin_nontemporal_load(in.p[a] + base + ij);
        }
        if constexpr (kWeights) wij = w[i] * w[j];
    }

    for (int t = tid; t < n * n; t += kBlock) s_D[t] = D_hat[t];
    __syncthreads(); // s_D is written across elements

    double D_i[nd], D_j[nd], Dt_i[nd], Dt_j[nd];
    if (kDReg)
    {
#pragma unroll
        for (int p = 0; p < nd; p++)
        {
            D_i[p] = s_D[p + i * n]; // D[i][p]: d/dr
            D_j[p] = s_D[p + j * n]; // D[j][p]: d/ds
            if constexpr (kOp == kWdiv)
            {
                Dt_i[p] = s_D[i + p * n]; // D[p][i]: D_r^T
                Dt_j[p] = s_D[j + p * n]; // D[p][j]: D_s^T
            }
        }
    }

    Column acc = (Column)(0.0); // wdiv: out of this lane's column

    // not unrolled, as in the stiffness kernel: unrolled, the D_hat entries become loop-invariant register state
#pragma unroll 1
    for (int k = 0; k < n; k++)
    {
        double(*sc)[C::epb][C::slab] = s_c[k & 1];
        if (active)
        {
#pragma unroll
            for (int f = 0; f < nF; f++) sc[f][el][lpos] = col[f][k];
        }

        double v[3] = {vq[0], vq[1], vq[2]};
        if constexpr (kOp == kWdiv)
        {
            if (active && k + 1 < n)
            {
#pragma unroll
                for (int a = 0; a < 3; a++) vq[a] = __builtin_nontemporal_load(in.p[a] + base + (ij + (k + 1) * nn));
            }
        }

        // row k of D_hat: wave-uniform address -> scalar loads
        double Dk[n];
#pragma unroll
        for (int p = 0; p < n; p++) Dk[p] = D_hat[p + k * n];

        element_sync<kWaveLocal>();

        // d[f][b] = d field_f / d r_b at (i, j, k), summed over p = 0..n-1 from 0.0
        double d[nF][3];
#pragma unroll
        for (int f = 0; f < nF; f++) d[f][0] = d[f][1] = d[f][2] = 0.0;
#pragma unroll
        for (int p = 0; p < n; p++)
        {
            const double di = kDReg ? D_i[kDReg ? p : 0] : s_D[p + i * n];
            const double dj = kDReg ? D_j[kDReg ? p : 0] : s_D[p + j * n];
#pragma unroll
            for (int f = 0; f < nF; f++)
            {
                d[f][0] = __builtin_fma(di, sc[f][el][p + j * C::ld], d[f][0]);
                d[f][1] = __builtin_fma(dj, sc[f][el][i + p * C::ld], d[f][1]);
                d[f][2] = __builtin_fma(Dk[p], col[f][p], d[f][2]);
            }
        }

        // J[a][b] = d[a][b]; Cf = adj J, I = Cf / det = J^-1 (host/box_mesh.hpp: deform_isoparametric)
        double Cf[3][3];
        Cf[0][0] = d[1][1] * d[2][2] - d[1][2] * d[2][1];
        Cf[0][1] = d[0][2] * d[2][1] - d[0][1] * d[2][2];
        Cf[0][2] = d[0][1] * d[1][2] - d[0][2] * d[1][1];
        Cf[1][0] = d[1][2] * d[2][0] - d[1][0] * d[2][2];
        Cf[1][1] = d[0][0] * d[2][2] - d[0][2] * d[2][0];
        Cf[1][2] = d[0][2] * d[1][0] - d[0][0] * d[1][2];
        Cf[2][0] = d[1][0] * d[2][1] - d[1][1] * d[2][0];
        Cf[2][1] = d[0][1] * d[2][0] - d[0][0] * d[2][1];
        Cf[2][2] = d[0][0] * d[1][1] - d[0][1] * d[1][0];

        const int off = ij + k * nn;
        if constexpr (kOp == kMass)
        {
            const double det = d[0][0] * Cf[0][0] + d[0][1] * Cf[1][0] + d[0][2] * Cf[2][0];
            if (active) __builtin_nontemporal_store(wij * w[k] * det, out.p[0] + base + off);
        }
        if constexpr (kOp == kGrad)
        {
            const double det = d[0][0] * Cf[0][0] + d[0][1] * Cf[1][0] + d[0][2] * Cf[2][0];
            const double rdet = 1.0 / det;
            if (active)
            {
#pragma unroll
                for (int a = 0; a < 3; a++) __builtin_nontemporal_store((d[3][0] * Cf[0][a] + d[3][1] * Cf[1][a] + d[3][2] * Cf[2][a]) * rdet, out.p[a] + base + off);
            }
        }
        if constexpr (kOp == kWdiv)
        {
            const double w3 = wij * w[k];
            double F[3];
#pragma unroll
            for (int b = 0; b < 3; b++) F[b] = w3 * (Cf[b][0] * v[0] + Cf[b][1] * v[1] + Cf[b][2] * v[2]);

            // one buffer is enough: the next slab's F is written behind the sync above, which every lane reaches after its reads of this one
            if (active)
            {
                s_f[0][el][lpos] = F[0];
                s_f[1][el][lpos] = F[1];
            }
            element_sync<kWaveLocal>();

            double o_r = 0.0, o_s = 0.0;
#pragma unroll
            for (int p = 0; p < n; p++)
            {
                const double dti = kDReg ? Dt_i[kDReg ? p : 0] : s_D[i + p * n];
                const double dtj = kDReg ? Dt_j[kDReg ? p : 0] : s_D[j + p * n];
                o_r = __builtin_fma(dti, s_f[0][el][p + j * C::ld], o_r);
                o_s = __builtin_fma(dtj, s_f[1][el][i + p * C::ld], o_s);
            }
            acc[k] = acc[k] + (o_r + o_s);
            // out(i,j,m) += D[k][m] F_t(i,j,k)
#pragma unroll
            for (int m = 0; m < n; m++) acc[m] = __builtin_fma(Dk[m], F[2], acc[m]);
        }
    }

    if constexpr (kOp == kWdiv)
    {
        if (active)
        {
            double *op = out.p[0] + base;
#pragma unroll
            for (int k = 0; k < n; k++) __builtin_nontemporal_store(acc[k], op + (ij + k * nn));
        }
    }
}

template <int kOp>
int launch_field(const OutPtrs3 &out, const Ptrs3 &in, const Ptrs3 &X, const double *D_hat, const double *w, int num_elements, int n, void *stream)
{
    fdd_for_n<2, 16>(n, [&](auto nc) {
        using C = FieldCfg<decltype(nc)::value>;
        const int grid = (num_elements + C::epb - 1) / C::epb;
        hipLaunchKernelGGL((field_kernel<decltype(nc)::value, kOp>), dim3(grid), dim3(kBlock), 0, fdd_stream(stream), out, in, X, D_hat, w, num_elements);
    });
    FDD_LAUNCH_CHECK();
    return 0;
}

// What the three entries check in the same order, before any arithmetic on the sizes and before any output is touched:
// the degree (the element bound divides by (N+1)^3), then the count.  *run: there is something to launch.
int field_sizes(int num_elements, int poly_degree, bool *run)
{
    *run = false;
    if (poly_degree < 1 || poly_degree > 15)
    {
        fdd_set_error("field kernels support poly_degree 1..15, got %d", poly_degree);
        return FDD_ERR_UNSUPPORTED;
    }
    const long long n = poly_degree + 1;
    FDD_REQUIRE(num_elements >= 0);
    FDD_REQUIRE(num_elements < (1LL << 31) / (n * n * n));
    *run = num_elements > 0;
    return 0;
}

int three_pointers(Ptrs3 &to, const double *const from[3])
{
    FDD_REQUIRE(from != nullptr);
    for (int a = 0; a < 3; a++)
    {
        FDD_REQUIRE(from[a] != nullptr);
        to.p[a] = from[a];
    }
    return 0;
}

// no output is an input, and no two outputs are the same array
int no_alias(const OutPtrs3 &out, int num_out, const Ptrs3 &in, int num_in, const Ptrs3 &X)
{
    for (int o = 0; o < num_out; o++)
    {
        for (int a = 0; a < num_in; a++) FDD_REQUIRE(out.p[o] != in.p[a]);
        for (int a = 0; a < 3; a++) FDD_REQUIRE(out.p[o] != X.p[a]);
        for (int q = 0; q < o; q++) FDD_REQUIRE(out.p[o] != out.p[q]);
    }
    return 0;
}

// ---- surface weights and outward normals of listed element faces (fdd_field_surface) ----
// One workgroup per listed face, n*n active lanes: lane (a, b) owns the face point a + n b.  The face slab of x, y, z is
// staged in LDS (rows padded by one double), the two in-face derivatives X_a, X_b are D_hat contracted along a and b
// (explicit fused multiply-adds, as above), Nvec is their cross product in the order that points along the face's own
// reference direction, and |Nvec| w_a w_b is the surface weight.  The derivative across the face is not needed.
// 24 B read and 8 (area) + 24 (normal) B written per face point.
template <int n>
struct SurfaceCfg
{
    static constexpr int nn = n * n;
    static constexpr int block = ((nn + FDD_WAVE - 1) / FDD_WAVE) * FDD_WAVE;
    static constexpr int ld = n + 1;
};

template <int n>
__global__ __launch_bounds__(SurfaceCfg<n>::block) void field_surface_kernel(double *__restrict__ area, OutPtrs3 normal, Ptrs3 X, const double *__restrict__ D_hat, const double *__restrict__ w, const int *__restrict__ face_elem,
                                                                              const int *__restrict__ face_side, int num_elements)
{
    using C = SurfaceCfg<n>;
    constexpr int nn = C::nn;
    constexpr int n3 = nn * n;
    __shared__ double s_D[n * C::ld]; // rows padded like the slab's: lane (a, b) reads rows a and b
    __shared__ double s_x[3][n * C::ld];

    const int face = blockIdx.x;
    const int elem = face_elem[face], side = face_side[face];
    // the host layer validates the list; a face outside the arrays is left alone rather than read
    if (elem < 0 || elem >= num_elements || side < 0 || side > 5) return;
    const int axis = side >> 1, upper = side & 1;
    const int tid = threadIdx.x;
    const bool active = tid < nn;
    const int b = active ? tid / n : 0;
    const int a = active ? tid - b * n : 0;
    const int fixed = upper ? n - 1 : 0;
    // (a, b) = (j, k) on r-faces, (i, k) on s-faces, (i, j) on t-faces
    const int point = axis == 0 ? fixed + n * (a + n * b) : (axis == 1 ? a + n * (fixed + n * b) : a + n * (b + n * fixed));
    const size_t at = (size_t)elem * n3 + point;

    if (active)
    {
#pragma unroll
        for (int c = 0; c < 3; c++) s_x[c][a + b * C::ld] = X.p[c][at];
        s_D[a + b * C::ld] = D_hat[tid]; // D[b][a]
    }
    __syncthreads();

    double da[3] = {0.0, 0.0, 0.0}, db[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int p = 0; p < n; p++)
    {
        const double Da = s_D[p + a * C::ld], Db = s_D[p + b * C::ld];
#pragma unroll
        for (int c = 0; c < 3; c++)
        {
            da[c] = __builtin_fma(Da, s_x[c][p + b * C::ld], da[c]);
            db[c] = __builtin_fma(Db, s_x[c][a + p * C::ld], db[c]);
        }
    }
    // Nvec = X_s x X_t (r-faces), X_t x X_r (s-faces), X_r x X_s (t-faces): X_a x X_b, on s-faces X_b x X_a
    // (the negation is exact)
    const double flip = axis == 1 ? -1.0 : 1.0;
    const double N[3] = {flip * (da[1] * db[2] - da[2] * db[1]), flip * (da[2] * db[0] - da[0] * db[2]), flip * (da[0] * db[1] - da[1] * db[0])};
    const double mag = sqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
    if (!active) return;
    const size_t o = (size_t)face * nn + tid;
    area[o] = (w[a] * w[b]) * mag;
    if (normal.p[0] != nullptr)
    {
        const double sign = upper ? 1.0 : -1.0;
#pragma unroll
        for (int c = 0; c < 3; c++) normal.p[c][o] = sign * N[c] / mag;
    }
}

// ---- the convection term c . grad u (fdd_field_convect, fdd_field_weak_convect; the formulas are in fdd_hip.h) ----
// Both begin as the gradient kernel does: the k-columns of x, y, z (and, strong form, u) in registers, slab k of each in LDS,
// J and C = adj J per point.  With c of the slab (read per slab, the next one requested a slab ahead, as wdiv's v is)
// chat_b = sum_a C[b][a] c_a.  The strong form stores (sum_b chat_b du/dr_b) / det: 56 B read and 8 B written per point.
//
// The weak form keeps chat_r, chat_s, chat_t as three more register columns and then streams over the M = (3n+1)/2 fine
// t-slabs; the fine element (M^3 points a field) never exists.  Per fine slab q_t, with P (M x n) the interpolation to the
// Gauss points and P' = P D its derivative, both staged in LDS with rows padded by one double:
//   1. lane (i, j) contracts its columns along t: chat_b and u with row q_t of P, u with row q_t of P' (rows at a
//      wave-uniform address: scalar loads); five n x n slabs S in LDS
//   2. along r to M x n: T = P S for the five and T = P' S for u; item (q_r, j) = lane's ij + m n^2, m < ceil(M n / n^2) <= 2
//   3. along s to M x M: chat_b(q), u,_t = P T(P'_t u), u,_r = P T(P'_r u), u,_s = P' T(u); item (q_r, q_s), <= 3 a lane;
//      Y = w_qr w_qs w_qt sum_b chat_b(q) u,_b(q)
//   4. back along s, Z = P^T Y (M x n), and along r, v = P^T Z (n x n): one value per lane
//   5. acc[k] += P[q_t][k] v for the n entries of the lane's output column, stored once behind the last slab
// Four element syncs a slab; each buffer is written a sync behind its last read.  The phase that forms chat uses the front of
// the same LDS (its two slab buffers of x, y, z are smaller than S).  The x, y, z columns are dead when the u column is
// read, so at most six columns are live (n = 16: 192 registers).
enum ConvectForm
{
    kStrong = 0,
    kWeak = 1
};

template <int n>
struct ConvectCfg
{
    using F = FieldCfg<n>;
    static constexpr int nn = n * n;
    static constexpr int M = (3 * n + 1) / 2;                 // Gauss points per direction
    static constexpr int r1 = (M * n + nn - 1) / nn;          // (q_r, j) items a lane
    static constexpr int r2 = (M * M + nn - 1) / nn;          // (q_r, q_s) items a lane
    static constexpr int ldp = n + 1;                         // padded row of P and P' in LDS
    static constexpr int oT = 5 * F::slab, oY = oT + 6 * M * n, oZ = oY + M * M;
    static constexpr int weak_doubles = oZ + M * n;           // S, T, Y, Z of an element
    static constexpr int strong_doubles = 2 * 4 * F::slab;    // two buffers of the slabs of x, y, z, u
};

template <int n, int kForm>
__global__ __launch_bounds__(kBlock) void convect_kernel(double *__restrict__ out, Ptrs3 cv, const double *__restrict__ u, Ptrs3 X, const double *__restrict__ D_hat, const double *__restrict__ P, const double *__restrict__ Pd,
                                                         const double *__restrict__ gw, int num_elements)
{
    using C = FieldCfg<n>;
    using W = ConvectCfg<n>;
    using Column = typename ColumnOf<C::vl>::type;
    constexpr int nn = C::nn;
    constexpr int n3 = nn * n;
    constexpr int M = W::M;
    constexpr bool kWaveLocal = (64 % nn == 0);
    constexpr int nF = (kForm == kStrong) ? 4 : 3; // fields differentiated: x, y, z and, strong form, u
    constexpr int per_elem = (kForm == kStrong) ? W::strong_doubles : W::weak_doubles;
    constexpr int nP = (kForm == kWeak) ? M * W::ldp : 1;

    __shared__ double s_D[n * n];
    __shared__ double s_P[nP], s_Pd[nP], s_w[kForm == kWeak ? M : 1];
    __shared__ double s_e[C::epb][per_elem];

    constexpr bool kWaveIsElement = (nn == 64);
    const int tid = threadIdx.x;
    const int e_loc = kWaveIsElement ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid / nn;
    const int ij = tid - e_loc * nn;
    const int j = ij / n;
    const int i = ij - j * n;
    const int elem = blockIdx.x * C::epb + e_loc;
    const bool active = (e_loc < C::epb) && (elem < num_elements);
    const size_t base = active ? (size_t)elem * n3 : 0;
    const int el = active ? e_loc : 0;
    const int lpos = i + j * C::ld;
    double *const se = s_e[el];

    Column col[nF];
#pragma unroll
    for (int f = 0; f < nF; f++) col[f] = (Column)(0.0);
    double cq[3] = {0.0, 0.0, 0.0};
    if (active)
    {
#pragma unroll
        for (int f = 0; f < 3; f++)
        {
            const double *cp = X.p[f] + base;
#pragma unroll
            for (int k = 0; k < n; k++) col[f][k] = __builtin_nontemporal_load(cp + (ij + k * nn));
        }
        if constexpr (kForm == kStrong)
        {
            const double *up = u + base;
#pragma unroll
            for (int k = 0; k < n; k++) col[3][k] = __builtin_nontemporal_load(up + (ij + k * nn));
        }
#pragma unroll
        for (int a = 0; a < 3; a++) cq[a] = __builtin_nontemporal_load(cv.p[a] + base + ij);
    }

    for (int t = tid; t < n * n; t += kBlock) s_D[t] = D_hat[t];
    if constexpr (kForm == kWeak)
    {
        for (int t = tid; t < M * n; t += kBlock)
        {
            const int q = t / n, p = t - q * n;
            s_P[p + q * W::ldp] = P[t];
            s_Pd[p + q * W::ldp] = Pd[t];
        }
        for (int t = tid; t < M; t += kBlock) s_w[t] = gw[t];
    }
    __syncthreads(); // the tables are written across elements

    Column ch[kForm == kWeak ? 3 : 1]; // weak form: chat_r, chat_s, chat_t of this lane's column
#pragma unroll
    for (int b = 0; b < (kForm == kWeak ? 3 : 1); b++) ch[b] = (Column)(0.0);

#pragma unroll 1
    for (int k = 0; k < n; k++)
    {
        double *sc = se + (k & 1) * (nF * C::slab);
        if (active)
        {
#pragma unroll
            for (int f = 0; f < nF; f++) sc[f * C::slab + lpos] = col[f][k];
        }

        const double c[3] = {cq[0], cq[1], cq[2]};
        if (active && k + 1 < n)
        {
#pragma unroll
            for (int a = 0; a < 3; a++) cq[a] = __builtin_nontemporal_load(cv.p[a] + base + (ij + (k + 1) * nn));
        }

        // row k of D_hat: wave-uniform address -> scalar loads
        double Dk[n];
#pragma unroll
        for (int p = 0; p < n; p++) Dk[p] = D_hat[p + k * n];

        element_sync<kWaveLocal>();

        double d[nF][3];
#pragma unroll
        for (int f = 0; f < nF; f++) d[f][0] = d[f][1] = d[f][2] = 0.0;
#pragma unroll
        for (int p = 0; p < n; p++)
        {
            const double di = s_D[p + i * n];
            const double dj = s_D[p + j * n];
#pragma unroll
            for (int f = 0; f < nF; f++)
            {
                d[f][0] = __builtin_fma(di, sc[f * C::slab + p + j * C::ld], d[f][0]);
                d[f][1] = __builtin_fma(dj, sc[f * C::slab + i + p * C::ld], d[f][1]);
                d[f][2] = __builtin_fma(Dk[p], col[f][p], d[f][2]);
            }
        }

        // J[a][b] = d[a][b]; Cf = adj J as in field_kernel
        double Cf[3][3];
        Cf[0][0] = d[1][1] * d[2][2] - d[1][2] * d[2][1];
        Cf[0][1] = d[0][2] * d[2][1] - d[0][1] * d[2][2];
        Cf[0][2] = d[0][1] * d[1][2] - d[0][2] * d[1][1];
        Cf[1][0] = d[1][2] * d[2][0] - d[1][0] * d[2][2];
        Cf[1][1] = d[0][0] * d[2][2] - d[0][2] * d[2][0];
        Cf[1][2] = d[0][2] * d[1][0] - d[0][0] * d[1][2];
        Cf[2][0] = d[1][0] * d[2][1] - d[1][1] * d[2][0];
        Cf[2][1] = d[0][1] * d[2][0] - d[0][0] * d[2][1];
        Cf[2][2] = d[0][0] * d[1][1] - d[0][1] * d[1][0];

        double chat[3];
#pragma unroll
        for (int b = 0; b < 3; b++) chat[b] = Cf[b][0] * c[0] + Cf[b][1] * c[1] + Cf[b][2] * c[2];

        if constexpr (kForm == kStrong)
        {
            const double det = d[0][0] * Cf[0][0] + d[0][1] * Cf[1][0] + d[0][2] * Cf[2][0];
            if (active) __builtin_nontemporal_store((chat[0] * d[3][0] + chat[1] * d[3][1] + chat[2] * d[3][2]) / det, out + base + (ij + k * nn));
        }
        else
        {
#pragma unroll
            for (int b = 0; b < 3; b++) ch[b][k] = chat[b];
        }
    }

    if constexpr (kForm == kWeak)
    {
        Column uc = (Column)(0.0);
        if (active)
        {
            const double *up = u + base;
#pragma unroll
            for (int k = 0; k < n; k++) uc[k] = __builtin_nontemporal_load(up + (ij + k * nn));
        }
        double *const sS = se, *const sT = se + W::oT, *const sY = se + W::oY, *const sZ = se + W::oZ;
        Column acc = (Column)(0.0);

        element_sync<kWaveLocal>(); // S lies over the slabs the last k read

#pragma unroll 1
        for (int qt = 0; qt < M; qt++)
        {
            // rows q_t of P and P': wave-uniform address -> scalar loads
            double Pk[n], Pdk[n];
#pragma unroll
            for (int p = 0; p < n; p++)
            {
                Pk[p] = P[p + qt * n];
                Pdk[p] = Pd[p + qt * n];
            }
            const double wt = gw[qt];

            // 1. along t
            double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < n; k++)
            {
#pragma unroll
                for (int b = 0; b < 3; b++) a[b] = __builtin_fma(Pk[k], ch[b][k], a[b]);
                a[3] = __builtin_fma(Pk[k], uc[k], a[3]);
                a[4] = __builtin_fma(Pdk[k], uc[k], a[4]);
            }
            if (active)
            {
#pragma unroll
                for (int f = 0; f < 5; f++) sS[f * C::slab + lpos] = a[f];
            }
            element_sync<kWaveLocal>();

            // 2. along r: T[0..2] = P chat_b, T[3] = P u, T[4] = P (P'_t u), T[5] = P' u
#pragma unroll
            for (int m = 0; m < W::r1; m++)
            {
                const int id = ij + m * nn;
                if (id < M * n)
                {
                    const int jj = id / M, qr = id - jj * M;
                    double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int p = 0; p < n; p++)
                    {
                        const double pr = s_P[p + qr * W::ldp], pdr = s_Pd[p + qr * W::ldp];
                        const double s3 = sS[3 * C::slab + p + jj * C::ld];
#pragma unroll
                        for (int b = 0; b < 3; b++) t[b] = __builtin_fma(pr, sS[b * C::slab + p + jj * C::ld], t[b]);
                        t[3] = __builtin_fma(pr, s3, t[3]);
                        t[4] = __builtin_fma(pr, sS[4 * C::slab + p + jj * C::ld], t[4]);
                        t[5] = __builtin_fma(pdr, s3, t[5]);
                    }
                    if (active)
                    {
#pragma unroll
                        for (int f = 0; f < 6; f++) sT[f * (M * n) + id] = t[f];
                    }
                }
            }
            element_sync<kWaveLocal>();

            // 3. along s, and the product on the fine slab
#pragma unroll
            for (int m = 0; m < W::r2; m++)
            {
                const int id = ij + m * nn;
                if (id < M * M)
                {
                    const int qs = id / M, qr = id - qs * M;
                    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; // chat_r, chat_s, chat_t, u,_s, u,_t, u,_r
#pragma unroll
                    for (int p = 0; p < n; p++)
                    {
                        const double ps = s_P[p + qs * W::ldp], pds = s_Pd[p + qs * W::ldp];
#pragma unroll
                        for (int b = 0; b < 3; b++) v[b] = __builtin_fma(ps, sT[b * (M * n) + qr + p * M], v[b]);
                        v[3] = __builtin_fma(pds, sT[3 * (M * n) + qr + p * M], v[3]);
                        v[4] = __builtin_fma(ps, sT[4 * (M * n) + qr + p * M], v[4]);
                        v[5] = __builtin_fma(ps, sT[5 * (M * n) + qr + p * M], v[5]);
                    }
                    if (active) sY[id] = ((s_w[qr] * s_w[qs]) * wt) * (v[0] * v[5] + v[1] * v[3] + v[2] * v[4]);
                }
            }
            element_sync<kWaveLocal>();

            // 4. back along s ...
#pragma unroll
            for (int m = 0; m < W::r1; m++)
            {
                const int id = ij + m * nn;
                if (id < M * n)
                {
                    const int jj = id / M, qr = id - jj * M;
                    double z = 0.0;
#pragma unroll
                    for (int q = 0; q < M; q++) z = __builtin_fma(s_P[jj + q * W::ldp], sY[qr + q * M], z);
                    if (active) sZ[id] = z;
                }
            }
            element_sync<kWaveLocal>();

            // ... and along r
            double val = 0.0;
#pragma unroll
            for (int q = 0; q < M; q++) val = __builtin_fma(s_P[i + q * W::ldp], sZ[q + j * M], val);

            // 5. out(i, j, k) += P[q_t][k] v(i, j)
#pragma unroll
            for (int k = 0; k < n; k++) acc[k] = __builtin_fma(Pk[k], val, acc[k]);
        }

        if (active)
        {
            double *op = out + base;
#pragma unroll
            for (int k = 0; k < n; k++) __builtin_nontemporal_store(acc[k], op + (ij + k * nn));
        }
    }
}

} // namespace

extern "C" {

int fdd_field_convect(double *out, const double *const c[3], const double *u, const double *const xyz[3], const double *D_hat, int num_elements, int poly_degree, void *stream)
{
    bool run;
    if (int rc = field_sizes(num_elements, poly_degree, &run)) return rc;
    if (!run) return 0;
    FDD_REQUIRE(out != nullptr && u != nullptr && D_hat != nullptr);
    Ptrs3 cv, X;
    if (int rc = three_pointers(cv, c)) return rc;
    if (int rc = three_pointers(X, xyz)) return rc;
    const OutPtrs3 o = {{out, nullptr, nullptr}};
    if (int rc = no_alias(o, 1, cv, 3, X)) return rc;
    FDD_REQUIRE(out != u && out != D_hat);
    fdd_for_n<2, 16>(poly_degree + 1, [&](auto nc) {
        constexpr int nv = decltype(nc)::value;
        const int grid = (num_elements + FieldCfg<nv>::epb - 1) / FieldCfg<nv>::epb;
        hipLaunchKernelGGL((convect_kernel<nv, kStrong>), dim3(grid), dim3(kBlock), 0, fdd_stream(stream), out, cv, u, X, D_hat, nullptr, nullptr, nullptr, num_elements);
    });
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_field_weak_convect(double *out, const double *const c[3], const double *u, const double *const xyz[3], const double *D_hat, const double *P, const double *Pd, const double *gl_weights, int num_quad, int num_elements, int poly_degree,
                           void *stream)
{
    bool run;
    if (int rc = field_sizes(num_elements, poly_degree, &run)) return rc;
    const int n = poly_degree + 1; // every degree has an instance: none needs scratch (DESIGN section 16 has the table)
    FDD_REQUIRE(num_quad == (3 * n + 1) / 2);
    if (!run) return 0;
    FDD_REQUIRE(out != nullptr && u != nullptr && D_hat != nullptr && P != nullptr && Pd != nullptr && gl_weights != nullptr);
    Ptrs3 cv, X;
    if (int rc = three_pointers(cv, c)) return rc;
    if (int rc = three_pointers(X, xyz)) return rc;
    const OutPtrs3 o = {{out, nullptr, nullptr}};
    if (int rc = no_alias(o, 1, cv, 3, X)) return rc;
    FDD_REQUIRE(out != u && out != D_hat && out != P && out != Pd && out != gl_weights);
    fdd_for_n<2, 16>(n, [&](auto nc) {
        constexpr int nv = decltype(nc)::value;
        const int grid = (num_elements + FieldCfg<nv>::epb - 1) / FieldCfg<nv>::epb;
        hipLaunchKernelGGL((convect_kernel<nv, kWeak>), dim3(grid), dim3(kBlock), 0, fdd_stream(stream), out, cv, u, X, D_hat, P, Pd, gl_weights, num_elements);
    });
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_field_surface(double *area, double *const normal[3], const double *const xyz[3], const double *D_hat, const double *gll_weights, const int *face_elem, const int *face_side, int num_faces, int num_elements, int poly_degree, void *stream)
{
    bool run;
    if (int rc = field_sizes(num_elements, poly_degree, &run)) return rc;
    const long long n = poly_degree + 1;
    FDD_REQUIRE(num_faces >= 0);
    FDD_REQUIRE(num_faces < (1LL << 31) / (n * n));
    if (num_faces == 0) return 0;
    FDD_REQUIRE(run); // faces of no element
    FDD_REQUIRE(area != nullptr && D_hat != nullptr && gll_weights != nullptr && face_elem != nullptr && face_side != nullptr);
    OutPtrs3 nrm = {{nullptr, nullptr, nullptr}};
    Ptrs3 X;
    if (int rc = three_pointers(X, xyz)) return rc;
    const void *outs[4] = {area, nullptr, nullptr, nullptr};
    int num_out = 1;
    if (normal != nullptr)
        for (int a = 0; a < 3; a++)
        {
            FDD_REQUIRE(normal[a] != nullptr);
            outs[num_out++] = nrm.p[a] = normal[a];
        }
    // no output is an input, and no two outputs are the same array
    const void *const ins[7] = {X.p[0], X.p[1], X.p[2], D_hat, gll_weights, face_elem, face_side};
    for (int o = 0; o < num_out; o++)
    {
        for (const void *in : ins) FDD_REQUIRE(outs[o] != in);
        for (int q = 0; q < o; q++) FDD_REQUIRE(outs[o] != outs[q]);
    }
    fdd_for_n<2, 16>((int)n, [&](auto nc) {
        constexpr int nv = decltype(nc)::value;
        hipLaunchKernelGGL((field_surface_kernel<nv>), dim3(num_faces), dim3(SurfaceCfg<nv>::block), 0, fdd_stream(stream), area, nrm, X, D_hat, gll_weights, face_elem, face_side, num_elements);
    });
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_field_mass(double *mass, const double *const xyz[3], const double *D_hat, const double *gll_weights, int num_elements, int poly_degree, void *stream)
{
    bool run;
    if (int rc = field_sizes(num_elements, poly_degree, &run)) return rc;
    if (!run) return 0;
    FDD_REQUIRE(mass != nullptr && D_hat != nullptr && gll_weights != nullptr);
    OutPtrs3 out = {{mass, nullptr, nullptr}};
    Ptrs3 in = {{nullptr, nullptr, nullptr}}, X;
    if (int rc = three_pointers(X, xyz)) return rc;
    if (int rc = no_alias(out, 1, in, 0, X)) return rc;
    return launch_field<kMass>(out, in, X, D_hat, gll_weights, num_elements, poly_degree + 1, stream);
}

int fdd_field_gradient(double *const grad[3], const double *u, const double *const xyz[3], const double *D_hat, int num_elements, int poly_degree, void *stream)
{
    bool run;
    if (int rc = field_sizes(num_elements, poly_degree, &run)) return rc;
    if (!run) return 0;
    FDD_REQUIRE(grad != nullptr && u != nullptr && D_hat != nullptr);
    OutPtrs3 out;
    for (int a = 0; a < 3; a++)
    {
        FDD_REQUIRE(grad[a] != nullptr);
        out.p[a] = grad[a];
    }
    Ptrs3 in = {{u, nullptr, nullptr}}, X;
    if (int rc = three_pointers(X, xyz)) return rc;
    if (int rc = no_alias(out, 3, in, 1, X)) return rc;
    return launch_field<kGrad>(out, in, X, D_hat, nullptr, num_elements, poly_degree + 1, stream);
}

int fdd_field_weak_divergence(double *out_, const double *const v[3], const double *const xyz[3], const double *D_hat, const double *gll_weights, int num_elements, int poly_degree, void *stream)
{
    bool run;
    if (int rc = field_sizes(num_elements, poly_degree, &run)) return rc;
    if (!run) return 0;
    FDD_REQUIRE(out_ != nullptr && D_hat != nullptr && gll_weights != nullptr);
    OutPtrs3 out = {{out_, nullptr, nullptr}};
    Ptrs3 in, X;
    if (int rc = three_pointers(in, v)) return rc;
    if (int rc = three_pointers(X, xyz)) return rc;
    if (int rc = no_alias(out, 1, in, 3, X)) return rc;
    return launch_field<kWdiv>(out, in, X, D_hat, gll_weights, num_elements, poly_degree + 1, stream);
}

} // extern "C"
