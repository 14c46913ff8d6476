// Matrix-free SEM stiffness Au = D^T G D u on GLL points, gfx950.
// Replaces domain.okl:5-98 (uniform degree) and subdomain.okl:4-101 (mixed
// degree with per-point indirection).
//
// (1) Reference two-launch form (stiffness_matrix_1 / _2, one lane per point,
//     global scratch GDu): kept for API parity and for degrees above 15.
//     112 B/point of HBM traffic (72 in 2-D).
//
// (2) Fused kernel (fdd_dom_stiffness_matrix / fdd_sub_stiffness_matrix):
//     64 B/point (u 8 + six geometric factors 48 + Au 8).  An element of
//     n = N+1 points per edge is owned by n*n lanes, lane (i,j) keeps its
//     k-column of u in registers.  For each k-slab the slab of u and then the
//     slabs of G*Du are staged through LDS (rows padded by one double: bank
//     conflict free for 8-B reads), x/y contractions read LDS, the z
//     contraction stays in registers.  With n = 8 an element is exactly one
//     64-lane wavefront and a 256-lane workgroup holds four elements.
//
//     Every output keeps the reference's operation order: Du_d and Au_d are
//     summed over p = 0..n-1 from 0.0, G*Du is evaluated left to right,
//     Au = (Au_1 + Au_2) + Au_3.  With -ffp-contract=off the fused kernel is
//     bit-identical to the two-launch form and to the OCCA-Serial arithmetic.
//
// Both are HBM-bound: 12n+17 flop/point is 1.77 flop/B at N=7.
#include "fdd_common.h"

namespace
{

constexpr int kBlock = 256;

template <typename T>
struct GPtrsT
{
    const T *g[FDD_NUM_GEOM_FACTS];
};

struct GPtrs
{
    const double *g[FDD_NUM_GEOM_FACTS];
};
struct GDuPtrs
{
    double *g[3];
};
struct LevelTable
{
    const double *D_hat[16];
    int poly_degree[16];
};

// ---------------------------------------------------------------------------
// (1) reference form, uniform degree: domain.okl:5-52 / :54-98
// ---------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(kBlock) void dom_stiffness_1_kernel(GDuPtrs GDu, const double *__restrict__ u, const double *__restrict__ D_hat, GPtrs G, int num_points, int n_x)
{
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= num_points) return;

    const int n_xy = n_x * n_x;
    const int num_elem_points = (DIM == 2) ? n_xy : n_xy * n_x;
    const int e = idx / num_elem_points;
    const int v = idx % num_elem_points;
    const double *ue = u + (size_t)e * num_elem_points;

    if (DIM == 2)
    {
        const int i = v % n_x;
        const int j = v / n_x;
        double Du_1 = 0.0, Du_2 = 0.0;
        for (int k = 0; k < n_x; k++)
        {
            Du_1 += D_hat[k + i * n_x] * ue[k + j * n_x];
            Du_2 += D_hat[k + j * n_x] * ue[i + k * n_x];
        }
        GDu.g[0][idx] = G.g[0][idx] * Du_1 + G.g[2][idx] * Du_2;
        GDu.g[1][idx] = G.g[2][idx] * Du_1 + G.g[1][idx] * Du_2;
    }
    else
    {
        const int i = v % n_x;
        const int j = (v / n_x) % n_x;
        const int k = v / n_xy;
        double Du_1 = 0.0, Du_2 = 0.0, Du_3 = 0.0;
        for (int p = 0; p < n_x; p++)
        {
            Du_1 += D_hat[p + i * n_x] * ue[p + j * n_x + k * n_xy];
            Du_2 += D_hat[p + j * n_x] * ue[i + p * n_x + k * n_xy];
            Du_3 += D_hat[p + k * n_x] * ue[i + j * n_x + p * n_xy];
        }
        GDu.g[0][idx] = G.g[0][idx] * Du_1 + G.g[3][idx] * Du_2 + G.g[4][idx] * Du_3;
        GDu.g[1][idx] = G.g[3][idx] * Du_1 + G.g[1][idx] * Du_2 + G.g[5][idx] * Du_3;
        GDu.g[2][idx] = G.g[4][idx] * Du_1 + G.g[5][idx] * Du_2 + G.g[2][idx] * Du_3;
    }
}

template <int DIM>
__global__ __launch_bounds__(kBlock) void dom_stiffness_2_kernel(double *__restrict__ Au, GDuPtrs GDu, const double *__restrict__ D_hat, int num_points, int n_x)
{
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= num_points) return;

    const int n_xy = n_x * n_x;
    const int num_elem_points = (DIM == 2) ? n_xy : n_xy * n_x;
    const int e = idx / num_elem_points;
    const int v = idx % num_elem_points;
    const size_t o = (size_t)e * num_elem_points;

    if (DIM == 2)
    {
        const int i = v % n_x;
        const int j = v / n_x;
        double Au_1 = 0.0, Au_2 = 0.0;
        for (int k = 0; k < n_x; k++)
        {
            Au_1 += D_hat[i + k * n_x] * GDu.g[0][o + (k + j * n_x)];
            Au_2 += D_hat[j + k * n_x] * GDu.g[1][o + (i + k * n_x)];
        }
        Au[idx] = Au_1 + Au_2;
    }
    else
    {
        const int i = v % n_x;
        const int j = (v / n_x) % n_x;
        const int k = v / n_xy;
        double Au_1 = 0.0, Au_2 = 0.0, Au_3 = 0.0;
        for (int p = 0; p < n_x; p++)
        {
            Au_1 += D_hat[i + p * n_x] * GDu.g[0][o + (p + j * n_x + k * n_xy)];
            Au_2 += D_hat[j + p * n_x] * GDu.g[1][o + (i + p * n_x + k * n_xy)];
            Au_3 += D_hat[k + p * n_x] * GDu.g[2][o + (i + j * n_x + p * n_xy)];
        }
        Au[idx] = Au_1 + Au_2 + Au_3;
    }
}

// ---------------------------------------------------------------------------
// (1') reference form, per-point indirection: subdomain.okl:4-53 / :55-101
// ---------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(kBlock) void sub_stiffness_1_kernel(GDuPtrs GDu, const double *__restrict__ u, LevelTable T, const int *__restrict__ offset, const int *__restrict__ vert, const int *__restrict__ level, GPtrs G, int num_points)
{
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= num_points) return;

    const int o = offset[idx];
    const int v = vert[idx];
    const int l = level[idx];
    const int n_x = T.poly_degree[l] + 1;
    const int n_xy = n_x * n_x;
    const double *D_hat = T.D_hat[l];

    if (DIM == 2)
    {
        const int i = v % n_x;
        const int j = v / n_x;
        double Du_1 = 0.0, Du_2 = 0.0;
        for (int k = 0; k < n_x; k++)
        {
            Du_1 += D_hat[k + i * n_x] * u[o + (k + j * n_x)];
            Du_2 += D_hat[k + j * n_x] * u[o + (i + k * n_x)];
        }
        GDu.g[0][idx] = G.g[0][idx] * Du_1 + G.g[2][idx] * Du_2;
        GDu.g[1][idx] = G.g[2][idx] * Du_1 + G.g[1][idx] * Du_2;
    }
    else
    {
        const int i = v % n_x;
        const int j = (v / n_x) % n_x;
        const int k = v / n_xy;
        double Du_1 = 0.0, Du_2 = 0.0, Du_3 = 0.0;
        for (int p = 0; p < n_x; p++)
        {
            Du_1 += D_hat[p + i * n_x] * u[o + (p + j * n_x + k * n_xy)];
            Du_2 += D_hat[p + j * n_x] * u[o + (i + p * n_x + k * n_xy)];
            Du_3 += D_hat[p + k * n_x] * u[o + (i + j * n_x + p * n_xy)];
        }
        GDu.g[0][idx] = G.g[0][idx] * Du_1 + G.g[3][idx] * Du_2 + G.g[4][idx] * Du_3;
        GDu.g[1][idx] = G.g[3][idx] * Du_1 + G.g[1][idx] * Du_2 + G.g[5][idx] * Du_3;
        GDu.g[2][idx] = G.g[4][idx] * Du_1 + G.g[5][idx] * Du_2 + G.g[2][idx] * Du_3;
    }
}

template <int DIM>
__global__ __launch_bounds__(kBlock) void sub_stiffness_2_kernel(double *__restrict__ Au, GDuPtrs GDu, LevelTable T, const int *__restrict__ offset, const int *__restrict__ vert, const int *__restrict__ level, int num_points)
{
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= num_points) return;

    const int o = offset[idx];
    const int v = vert[idx];
    const int l = level[idx];
    const int n_x = T.poly_degree[l] + 1;
    const int n_xy = n_x * n_x;
    const double *D_hat = T.D_hat[l];

    if (DIM == 2)
    {
        const int i = v % n_x;
        const int j = v / n_x;
        double Au_1 = 0.0, Au_2 = 0.0;
        for (int k = 0; k < n_x; k++)
        {
            Au_1 += D_hat[i + k * n_x] * GDu.g[0][o + (k + j * n_x)];
            Au_2 += D_hat[j + k * n_x] * GDu.g[1][o + (i + k * n_x)];
        }
        Au[idx] = Au_1 + Au_2;
    }
    else
    {
        const int i = v % n_x;
        const int j = (v / n_x) % n_x;
        const int k = v / n_xy;
        double Au_1 = 0.0, Au_2 = 0.0, Au_3 = 0.0;
        for (int p = 0; p < n_x; p++)
        {
            Au_1 += D_hat[i + p * n_x] * GDu.g[0][o + (p + j * n_x + k * n_xy)];
            Au_2 += D_hat[j + p * n_x] * GDu.g[1][o + (i + p * n_x + k * n_xy)];
            Au_3 += D_hat[k + p * n_x] * GDu.g[2][o + (i + j * n_x + p * n_xy)];
        }
        Au[idx] = Au_1 + Au_2 + Au_3;
    }
}

// ---------------------------------------------------------------------------
// (2) fused kernel, 3-D, n = N+1 in [2, 16]
// ---------------------------------------------------------------------------
template <int n>
struct FusedCfg
{
    static constexpr int nn = n * n;
    static constexpr int epb = (kBlock / nn) > 0 ? (kBlock / nn) : 1; // elements per workgroup
    static constexpr int ld = n + 1;                                  // padded LDS row
    static constexpr int slab = n * ld;
};

// Synchronisation between the LDS phases of one element.  When n*n divides 64
// an element never straddles a wavefront (n = 2, 4, 8: the headline N = 7), the
// LDS executes a wave's instructions in order, and no barrier is needed at all:
// every wave streams its elements independently.  Otherwise a barrier that
// waits on the LDS counter only -- __syncthreads() would also drain the vector
// memory counter, i.e. the geometric factors prefetched for the next slab.
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

// kGather: u is read through point_dof (u[e,i,j,k] = v[point_dof[...]], 0 where
// the point has no dof): the boolean scatter Q of Subdomain fused into the load.
// T: double, or float for the single-precision preconditioner (the reference's PTYPE = Float, config.hpp:19-20)
// kAffine: the six factors of a point are NOT streamed (48 of the 64 B per point) but formed from six numbers per element
// and the GLL weights, G_f(e; i, j, k) = c_f(e) * (w_i w_j) w_k -- what they are on an element that is an affine image
// of the reference cube (every element of a box mesh).  G.g[0] then points to c (element-major, 6 per element of this
// list), G.g[1] to the n weights.  An option of this build (the reference always streams G): the host layer offers it
// only where the mesh's own factor arrays satisfy the product form to rounding (host/element.hpp: affine_factors).
// kDiag: the three off-diagonal factor arrays G.g[3..5] are NOT streamed (24 of the 64 B per point): the caller has
// established that they are 0.0 at every point of the list (fdd_stiffness_offdiag_zero; every mesh whose elements have
// orthogonal axes), and GDu_d = g[d] * Du_d.  What is left out is the addition of exact zeros: every output is the IEEE
// value the six-array kernel gives, for finite u, up to the sign of a zero.  Three factor registers per slab in flight: the
// double gather instance at n = 8 takes 131 VGPRs (148 with six arrays), 3 waves per SIMD, no scratch, 136 us per launch at
// 32^3 elements against 170.  A launch bound of 4 waves (126 VGPRs) and kPF = 2 (144 VGPRs) both measured 134-136 us, inside
// the spread; kPF = 2 under the bound of 4 spills.
template <typename T, int n, bool kGather, bool kNTStore, bool kAffine = false, bool kDiag = false>
__global__ __launch_bounds__(kBlock, (kAffine && n == 8 && sizeof(T) == 8) ? 4 : 1) void fused_stiffness_kernel_t(T *__restrict__ Au, const T *__restrict__ u, const int *__restrict__ point_dof, const double *__restrict__ u_scale, const T *__restrict__ D_hat, GPtrsT<T> G, const int *__restrict__ elem_offset, int num_elements)
{
    using C = FusedCfg<n>;
    constexpr int nn = C::nn;
    constexpr int n3 = nn * n;
    constexpr bool kWaveLocal = (64 % nn == 0);
    // D_hat rows/columns a lane needs in every slab live in registers up to
    // n = 8 (4 x 8 doubles); above that they are re-read from LDS per slab.
    constexpr bool kDReg = (n <= 8);
    constexpr int nd = kDReg ? n : 1;

    __shared__ T s_D[n * n];
    __shared__ T s_u[C::epb][n * C::slab];   // the element, rows padded; slab k is reused for Au_1 + Au_2 once consumed
    __shared__ T s_g[2][2][C::epb][C::slab]; // GDu_1 / GDu_2 of the slab, T buffered: one sync per slab

    // n = 8: the element index is the wavefront index.  Telling the compiler so
    // (readfirstlane) keeps the element base, the `active` test and all array
    // bases in scalar registers: loads take the SGPR-base + 32-bit lane offset form.
    constexpr bool kWaveIsElement = (nn == 64);
    const int tid = threadIdx.x;
    const int e_loc = kWaveIsElement ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid / nn;
    const int ij = tid - e_loc * nn;
    const int j = ij / n;
    const int i = ij - j * n;
    const int elem = blockIdx.x * C::epb + e_loc;
    const bool active = (e_loc < C::epb) && (elem < num_elements);

    size_t base = 0;
    if (active) base = elem_offset ? (size_t)elem_offset[elem] : (size_t)elem * n3;

    const int el = active ? e_loc : 0;
    T *su = s_u[el];
    const int lpos = i + j * C::ld;

    // this lane's k-column of u: registers for the z contraction, LDS for x and y;
    // geometric factors of the first kPF slabs right behind it (inside the loop slab
    // k + kPF is requested as soon as slab k's are consumed).  All of it is in
    // flight before D_hat is staged.
    constexpr int kPF = 1; // slabs of geometric factors in flight (2 measured no faster at n = 8, with six arrays and with three: the kernel is not latency-bound)
    constexpr int nG = kDiag ? 3 : FDD_NUM_GEOM_FACTS;                          // factor arrays streamed
    T r_u[n], r_3[n], gq[kPF][nG];
    T cf[FDD_NUM_GEOM_FACTS], wij = T(0); // kAffine: the element's six numbers, w_i w_j of this lane
#pragma unroll
    for (int f = 0; f < FDD_NUM_GEOM_FACTS; f++) cf[f] = T(0);
#pragma unroll
    for (int k = 0; k < n; k++) r_u[k] = T(0);
#pragma unroll
    for (int s = 0; s < kPF; s++)
#pragma unroll
        for (int f = 0; f < nG; f++) gq[s][f] = T(0);
    if (active)
    {
        if (kGather)
        {
            const int *pd = point_dof + base;
            int d[n];
#pragma unroll
            for (int k = 0; k < n; k++) d[k] = __builtin_nontemporal_load(pd + (ij + k * nn));
            // unconditional loads on a selected index (dof 0 stands in where the point has none): a load
            // under a lane predicate becomes a branch with its own wait and the n loads serialise
#pragma unroll
            for (int k = 0; k < n; k++) r_u[k] = u[d[k] < 0 ? 0 : d[k]];
#pragma unroll
            for (int k = 0; k < n; k++) r_u[k] = (d[k] < 0) ? T(0) : r_u[k];
            if (u_scale) // v stands for (*u_scale) * v: a Krylov vector kept unnormalised (math.okl:29-35 applied on load)
            {
                const T sc = (T)(*u_scale);
#pragma unroll
                for (int k = 0; k < n; k++) r_u[k] = sc * r_u[k];
            }
        }
        else
        {
            const T *up = u + base;
#pragma unroll
            for (int k = 0; k < n; k++) r_u[k] = __builtin_nontemporal_load(up + (ij + k * nn));
        }
        if (kAffine)
        {
#pragma unroll
            for (int f = 0; f < FDD_NUM_GEOM_FACTS; f++) cf[f] = G.g[0][(size_t)elem * FDD_NUM_GEOM_FACTS + f];
            wij = G.g[1][i] * G.g[1][j];
        }
        else
        {
#pragma unroll
            for (int s = 0; s < kPF; s++)
#pragma unroll
                for (int f = 0; f < nG; f++) gq[s][f] = __builtin_nontemporal_load(G.g[f] + base + (ij + s * nn));
        }
    }

    for (int t = tid; t < n * n; t += kBlock) s_D[t] = D_hat[t];

#pragma unroll
    for (int k = 0; k < n; k++) r_3[k] = T(0);
    if (active)
    {
#pragma unroll
        for (int k = 0; k < n; k++) su[lpos + k * C::slab] = r_u[k];
    }

    __syncthreads(); // s_D (written across elements) and s_u

    T D_i[nd], D_j[nd], Dt_i[nd], Dt_j[nd];
    if (kDReg)
    {
#pragma unroll
        for (int p = 0; p < nd; p++)
        {
            D_i[p] = s_D[p + i * n];  // D_hat[p + i*n_x]: pass 1, x
            D_j[p] = s_D[p + j * n];  // D_hat[p + j*n_x]: pass 1, y
            Dt_i[p] = s_D[i + p * n]; // D_hat[i + p*n_x]: pass 2, x
            Dt_j[p] = s_D[j + p * n]; // D_hat[j + p*n_x]: pass 2, y
        }
    }

    // The slab loop is deliberately NOT unrolled beyond the prefetch depth:
    // unrolled, every D_hat entry becomes loop-invariant register state
    // (> 256 VGPRs and scratch spills).  A wave waits one full HBM latency per
    // slab unless enough slabs of geometric factors are already requested:
    // kPF slabs are in flight per lane (12 VGPRs each).
#pragma unroll 1
    for (int k0 = 0; k0 < n; k0 += kPF)
    {
#pragma unroll
        for (int s = 0; s < kPF; s++)
        {
            const int k = k0 + s;
            if ((n % kPF != 0) && k >= n) continue;
            // this slot's factors move to g; slab k + kPF is requested into the slot
            T g[kAffine ? FDD_NUM_GEOM_FACTS : nG];
            if (kAffine)
            {
                const T w3 = wij * G.g[1][k]; // w_k: wave-uniform address
#pragma unroll
                for (int f = 0; f < FDD_NUM_GEOM_FACTS; f++) g[f] = cf[f] * w3;
            }
            else
            {
#pragma unroll
                for (int f = 0; f < nG; f++) g[f] = gq[s][f];
            }
            if (!kAffine && active && k + kPF < n)
            {
                const int off = ij + (k + kPF) * nn;
#pragma unroll
                for (int f = 0; f < nG; f++) gq[s][f] = __builtin_nontemporal_load(G.g[f] + base + off);
            }

            // row k of D_hat: wave-uniform address -> scalar loads, lives in SGPRs
            T Dk[n];
#pragma unroll
            for (int p = 0; p < n; p++) Dk[p] = D_hat[p + k * n];

            // opaque copies of i, j stop the compiler from hoisting the D_hat LDS
            // reads out of the slab loop when they are not meant to be registers
            int io = i, jo = j;
            if (!kDReg) asm volatile("" : "+v"(io), "+v"(jo));

            const T *suk = su + k * C::slab;
            T Du_1 = T(0), Du_2 = T(0), Du_3 = T(0);
#pragma unroll
            for (int p = 0; p < n; p++)
            {
                const T di = kDReg ? D_i[kDReg ? p : 0] : s_D[p + io * n];
                const T dj = kDReg ? D_j[kDReg ? p : 0] : s_D[p + jo * n];
                Du_1 += di * suk[p + j * C::ld];
                Du_2 += dj * suk[i + p * C::ld];
                Du_3 += Dk[p] * r_u[p];
            }

            T GDu_1, GDu_2, GDu_3;
            if constexpr (kDiag)
            {
                GDu_1 = g[0] * Du_1;
                GDu_2 = g[1] * Du_2;
                GDu_3 = g[2] * Du_3;
            }
            else
            {
                GDu_1 = g[0] * Du_1 + g[3] * Du_2 + g[4] * Du_3;
                GDu_2 = g[3] * Du_1 + g[1] * Du_2 + g[5] * Du_3;
                GDu_3 = g[4] * Du_1 + g[5] * Du_2 + g[2] * Du_3;
            }

            T *sg1 = s_g[k & 1][0][el];
            T *sg2 = s_g[k & 1][1][el];
            if (active)
            {
                sg1[lpos] = GDu_1;
                sg2[lpos] = GDu_2;
            }
            element_sync<kWaveLocal>();

            T Au_1 = T(0), Au_2 = T(0);
#pragma unroll
            for (int p = 0; p < n; p++)
            {
                const T dti = kDReg ? Dt_i[kDReg ? p : 0] : s_D[io + p * n];
                const T dtj = kDReg ? Dt_j[kDReg ? p : 0] : s_D[jo + p * n];
                Au_1 += dti * sg1[p + j * C::ld];
                Au_2 += dtj * sg2[i + p * C::ld];
            }
            // every lane of the element is past its reads of slab k of s_u (they
            // precede the sync above): the slot now holds Au_1 + Au_2 of this point
            if (active) su[lpos + k * C::slab] = Au_1 + Au_2;

            // Au_3(i,j,m) += D_hat[m + k*n_x] * GDu_3(i,j,k): the reference's p = k term
#pragma unroll
            for (int m = 0; m < n; m++) r_3[m] += Dk[m] * GDu_3;
        }
    }

    if (active)
    {
        // the s_u slots are read back by the lane that wrote them
        T *Aup = Au + base;
#pragma unroll
        for (int k = 0; k < n; k++)
        {
            const T v = su[lpos + k * C::slab] + r_3[k];
            if (kNTStore)
                __builtin_nontemporal_store(v, Aup + (ij + k * nn));
            else
                Aup[ij + k * nn] = v;
        }
    }
}

// FDD_TUNE_STIFFNESS_NT_STORE, read once
inline bool stiffness_nt_store()
{
    static const bool nt_store = fdd_env_int("FDD_TUNE_STIFFNESS_NT_STORE", 1) != 0;
    return nt_store;
}

// the instance of a kernel by (gather on load, non-temporal stores): f(gather, nt_store) with two std::bool_constant
template <typename F>
inline void for_gather_nt_store(const int *point_dof, F &&f)
{
    fdd_for_bool(point_dof != nullptr, [&](auto gather) { fdd_for_bool(stiffness_nt_store(), [&](auto nt) { f(gather, nt); }); });
}

// kDiag: the three-array instances; G.g[3..5] are not passed on (never dereferenced)
template <typename T, int n, bool kDiag>
int launch_fused_t(T *Au, const T *u, const int *point_dof, const double *u_scale, const T *D_hat, const GPtrsT<T> &G, const int *elem_offset, int num_elements, void *stream)
{
    using C = FusedCfg<n>;
    const int grid = (num_elements + C::epb - 1) / C::epb;
    for_gather_nt_store(point_dof, [&](auto gather, auto nt) {
        hipLaunchKernelGGL((fused_stiffness_kernel_t<T, n, decltype(gather)::value, decltype(nt)::value, false, kDiag>), dim3(grid), dim3(kBlock), 0, fdd_stream(stream), Au, u, point_dof, u_scale, D_hat, G, elem_offset, num_elements);
    });
    FDD_LAUNCH_CHECK();
    return 0;
}

// six factor arrays or, kDiag, three; in double or in float (the single-precision form is used gather-on-load only: the
// preconditioner's dof-space solve, and has no two-launch form to point to)
template <typename T, bool kDiag = false>
int fused_dispatch(T *Au, const T *u, const int *point_dof, const double *u_scale, const T *D_hat, const T *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream)
{
    FDD_REQUIRE(num_elements >= 0);
    if (num_elements == 0) return 0;
    FDD_REQUIRE(Au != nullptr && u != nullptr && D_hat != nullptr && G != nullptr);
    GPtrsT<T> g;
    if constexpr (kDiag)
    {
        if (int rc = fdd_three_factors(g, G)) return rc;
    }
    else
        for (int k = 0; k < FDD_NUM_GEOM_FACTS; k++)
        {
            FDD_REQUIRE(G[k] != nullptr);
            g.g[k] = G[k];
        }
    int rc = 0;
    if (fdd_for_n<2, 16>(poly_degree + 1, [&](auto n) { rc = launch_fused_t<T, decltype(n)::value, kDiag>(Au, u, point_dof, u_scale, D_hat, g, elem_offset, num_elements, stream); })) return rc;
    if constexpr (sizeof(T) == 4 && !kDiag)
        fdd_set_error("fused stiffness kernel supports poly_degree 1..15, got %d", poly_degree);
    else
        fdd_set_error("fused stiffness kernel supports poly_degree 1..15, got %d (use the two-launch form)", poly_degree);
    return FDD_ERR_UNSUPPORTED;
}

// ---------------------------------------------------------------------------
// (2b) line form of the three-array fused kernel, 3-D, n = 8 only
// ---------------------------------------------------------------------------
// The same arithmetic as fused_stiffness_kernel_t<T, 8, ., ., false, true>, bit for bit, under another thread-to-data
// mapping.  An element is one wavefront, and lane l = a + 8 b plays three roles in turn:
//   (i, j) = (a, b)  owns the k-column: coalesced loads of u / the index gather, the z contraction, the final sum, the store;
//   (j, k) = (a, b)  owns the x-row    u(0..7, j, k);
//   (i, k) = (a, b)  owns the y-column u(i, 0..7, k).
// In each role the lane holds a whole line, so D u, g * (D u) and D^T (g D u) along it are register-only 8 x 8 mat-vecs
// with D_hat as a wave-uniform (scalar) operand: eight independent sums per pass, every one over p ascending from 0 as
// in the reference.  Both passes walk D_hat by rows (Du_i = sum_p D[p + 8 i] u_p has i outside; Au_i += D[i + 8 p] GDu_p
// has p outside), so no transposed table is needed.  LDS only transposes between the roles: 8 stores of u, 8 + 8 loads,
// 8 + 8 stores of the Au_1 / Au_2 lines, 8 + 8 loads = 56 accesses per lane and element (7 per point; the slab form: 34)
// in two round trips (the slab form: sixteen).  No workgroup barrier: a wave past the last element leaves at once.
//
// LDS tile of one element, in words of T: point (i, j, k) lives at  ((i + j) & 7) + 8 j + 72 k  -- rows of 8 rotated by
// their j, slabs 72 apart.  The LDS services 8-byte reads in lane groups of 32 over 32 double-wide banks and 8-byte
// writes in groups of 16 over 16 (MI355X: ds_read_b64 2 x 32 lanes, bank = (byte address / 4) mod 64; ds_write_b64
// 4 x 16 lanes, mod 32); for float the groups are 32 lanes over 32 banks both ways, the same arithmetic mod 32.  With
// r = (i + j) & 7 and s = (j + k) & 3 the bank of a point is r + 8 s (72 k = 8 k mod 32), and in every role the 8 values
// of a give 8 different r while the 4 values of b in a group give 4 different s (2 different s mod 2 in a write group):
//   k-column, k fixed:  r = (a + b) & 7 runs through 0..7 with a;  s = (b + k) & 3 with b;
//   x-row,    i = p:    r = (p + a) & 7 with a;                     s = (a + b) & 3 with b at fixed a, i.e. fixed r;
//   y-column, j = p:    r = (a + p) & 7 with a;                     s = (p + b) & 3 with b.
// So all six patterns (k-column store, x-row and y-column loads, the two line stores, the k-column load) are free of
// bank conflicts.  The x-row is not contiguous in LDS under the rotation: its loads are 8-byte, which run at the same
// 256 B per clock as 16-byte ones.  Au_1 has a tile of its own; the y-column role writes Au_2 over the u tile (every
// lane's loads of u precede those stores in the wave's instruction order, which the LDS keeps), so only one of the two
// lines of u is in registers at a time: 2 x 4.5 KiB per element in double, 36 KiB per workgroup, four workgroups per CU.
//
// Three arrays (kDiag): g[2] coalesced in k-column role, g[1] in y-column role (8 lanes x 8 B per 64-byte segment:
// sector-exact), g[0] in x-row role as 64 contiguous bytes per lane (plain loads, the lanes of a row share cache lines
// across them; loaded coalesced and transposed through LDS instead it measured 107.6 against 106.6 us per launch at 32^3
// elements in double and 69.5 against 65.0 in float, and was taken out).  Each role forms D u, g * (D u) and D^T (g D u)
// of its line without leaving registers: two LDS round trips per element.
// Six arrays: G Du mixes the three directions at a point, so Du_1 and Du_2 have to go back to the k-column role through
// the two tiles for the 3 x 3 combination (factors coalesced as in the slab form) and GDu_1 / GDu_2 out again to the row
// and column roles for D^T: four round trips, 15 accesses per point.  Built that way (84 VGPRs, 4 waves per SIMD, the
// same bits) it ran 172.9 us per launch at 32^3 elements against the slab form's 169.7 in double and 94.2 against 93.6
// in float -- that instance streams 1.10 GB and is at the memory system's rate already -- so the six-array lists keep
// the slab form and no six-array line instance is compiled.
struct LineCfg
{
    static constexpr int n = 8, nn = 64, n3 = 512;
    static constexpr int epb = kBlock / nn; // elements (waves) per workgroup
    static constexpr int slab = 72;
    static constexpr int tile = n * slab;
    __device__ static __forceinline__ int at(int i, int j, int k) { return ((i + j) & 7) + 8 * j + slab * k; }
};

// Row r of D_hat at an offset the compiler cannot see through (the offset, not the pointer: D_hat stays the read-only
// kernel argument that scalar loads need).  The kernel uses every row six times; read off the one
// kernel argument the 64 entries become 128 scalar registers that live from end to end, more than there are, and come
// back out of VGPR lanes one v_readlane per use.  Opaque, a row is 8 values in scalar registers for as long as its 16
// products last, re-read (scalar cache) by the next pass.
template <typename T>
__device__ __forceinline__ const T *line_row(const T *D_hat, int r)
{
    int at = 8 * r;
    asm volatile("" : "+s"(at));
    return D_hat + at;
}

// the two halves of a line's work, sums in the reference's order; D_hat is wave-uniform: scalar loads
template <typename T>
__device__ __forceinline__ void line_du(T (&du)[8], const T (&ul)[8], const T *__restrict__ D_hat) // du_i = sum_p D[p + 8 i] u_p
{
#pragma unroll
    for (int i = 0; i < 8; i++)
    {
        const T *Di = line_row(D_hat, i);
        du[i] = T(0);
#pragma unroll
        for (int p = 0; p < 8; p++) du[i] += Di[p] * ul[p];
    }
}
template <typename T>
__device__ __forceinline__ void line_au(T (&au)[8], const T (&gdu)[8], const T *__restrict__ D_hat) // au_i = sum_p D[i + 8 p] gdu_p
{
#pragma unroll
    for (int i = 0; i < 8; i++) au[i] = T(0);
#pragma unroll
    for (int p = 0; p < 8; p++)
    {
        const T *Dp = line_row(D_hat, p);
#pragma unroll
        for (int i = 0; i < 8; i++) au[i] += Dp[i] * gdu[p];
    }
}

// ---- the lean instances (kLean != 0; fdd_stiffness_matrix_lines_lean[_f32]) ----
// The caller guarantees two things about D_hat, bit for bit: the interior diagonal D_hat[i + 8 i], i = 1..6, is +-0.0, and
// D_hat[63 - m] = -D_hat[m] for every other m (both hold for the table of mirrored GLL nodes).  The lean instances then leave out
// work the value of the result does not need; each part is one bit of kLean:
//   kLeanTerms     every partial sum starts from its first product instead of T(0) +, and the products with an interior
//                  diagonal entry are left out; the remaining terms keep their ascending order.  120 of the 816
//                  floating-point instructions per lane.  What is dropped is the addition of exact zeros: for finite
//                  inputs the result is the parent's, to the sign of a zero.
//   kLeanResident  D_hat is read once at kernel entry: the 29 entries m < 32 off the diagonal, 58 scalar registers in
//                  double.  Entry m >= 32 is used as -D_hat[63 - m] (a source modifier on the multiply, the same bits as
//                  the stored entry).  The body has no scalar load, so no lgkmcnt(0) wait for one sits between its LDS
//                  accesses.  Needs kLeanTerms (the diagonal entries are not kept).
// Requesting the shared instance's factor lines ahead of the point_dof gather was built as a third part and measured no
// faster (HISTORY); it is not in the kernel.  In float the resident table measured no faster than the row loads either, so
// the float entries run kLeanTerms alone.
enum : int
{
    kLeanTerms = 1,
    kLeanResident = 2
};

// D_hat as the lean instances read it: entry (r, c) = D_hat[c + 8 r], r and c known at compile time after unrolling
template <typename T, bool kResident>
struct LeanTable
{
    static constexpr int slot(int m) { return m - (m > 9) - (m > 18) - (m > 27); } // m < 32 without the diagonal 9, 18, 27
    const T *D_hat;
    T d[kResident ? 29 : 1];
    __device__ __forceinline__ explicit LeanTable(const T *__restrict__ D) : D_hat(D)
    {
        if constexpr (kResident)
        {
            T top[32]; // rows 0..3 in a few wide scalar loads, all requested before the first is waited for
#pragma unroll
            for (int m = 0; m < 32; m++) top[m] = D[m];
#pragma unroll
            for (int m = 0; m < 32; m++)
                if (m != 9 and m != 18 and m != 27)
                {
                    T v = top[m];
                    asm volatile("" : "+s"(v)); // a scalar register from here on: not re-read, not moved into lanes
                    d[slot(m)] = v;
                }
        }
    }
    __device__ __forceinline__ const T *row(int r) const { return kResident ? nullptr : line_row(D_hat, r); }
    __device__ __forceinline__ T at(const T *row_r, int r, int c) const
    {
        if constexpr (kResident)
        {
            const int m = c + 8 * r;
            return m < 32 ? d[slot(m)] : -d[slot(63 - m)];
        }
        else
            return row_r[c];
    }
};
__device__ __forceinline__ constexpr bool lean_zero_entry(int r, int c) { return r == c and r >= 1 and r <= 6; }

// line_du / line_au without the zero terms: the first product starts the sum, the others follow in ascending order
template <typename T, bool kResident>
__device__ __forceinline__ void lean_du(T (&du)[8], const T (&ul)[8], const LeanTable<T, kResident> &D)
{
#pragma unroll
    for (int i = 0; i < 8; i++)
    {
        const T *Di = D.row(i);
        du[i] = D.at(Di, i, 0) * ul[0];
#pragma unroll
        for (int p = 1; p < 8; p++)
            if (not lean_zero_entry(i, p)) du[i] += D.at(Di, i, p) * ul[p];
    }
}
template <typename T, bool kResident>
__device__ __forceinline__ void lean_au(T (&au)[8], const T (&gdu)[8], const LeanTable<T, kResident> &D)
{
#pragma unroll
    for (int p = 0; p < 8; p++)
    {
        const T *Dp = D.row(p);
#pragma unroll
        for (int i = 0; i < 8; i++)
        {
            if (p == 0)
                au[i] = D.at(Dp, 0, i) * gdu[0];
            else if (not lean_zero_entry(p, i))
                au[i] += D.at(Dp, p, i) * gdu[p];
        }
    }
}

// kShared: element e reads its three factor lines from the block of element factor_elem[e] of the same arrays (the host
// layer establishes, from the list's own arrays, which elements hold bit for bit the block of an earlier one:
// fdd_stiffness_factor_block_hash / _verify).  The lookup is wave-uniform, so the factor base stays in scalar registers
// like the element's own; the factor loads are plain loads, since the few distinct blocks are meant to stay in cache
// (a nontemporal load goes past L1).  u, point_dof and Au keep the element's own base, and nothing else differs: the same
// words reach the same arithmetic.  factor_elem is not read by the streamed instances.
//
// kDirect (double, gather; fdd_stiffness_matrix_lines_direct): most of the values go straight to the rows of y = Qt Au they
// are the only or one of two entries of, instead of through the point buffer and the gather Qt.  point_dof carries, in the
// two bits above kDirectDofBits, what the host layer found in Qt's own arrays about the row of each point's dof:
//   general    anything else: the value goes to the point buffer Au as in the other instances, for the gather of those rows;
//   single     the row's only entry:                            y[dof] = T(0) + v;
//   pair-low   point (7, j, k) of element e, first of two entries: v is handed to the next wave through LDS;
//   pair-high  point (0, j, k) of element e + 1 of the same workgroup, second entry: y[dof] = (T(0) + left) + v;
// a negative entry is a point without a dof, which stores nothing.  The sums are the statements of the gather's row sum
// (s = T(0); s += 1.0 * x[j] in column order), so every bit is the one csr_short_pipelined_kernel would have written.  One
// workgroup barrier stands between the hand-over and its readers, so a wave past the last element does not leave early:
// it skips the element and meets the others at the barrier.  kDirect: 1 plain, 2 non-temporal stores of y.
constexpr int kDirectDofBits = 29;
constexpr int kDirectDofMask = (1 << kDirectDofBits) - 1;
enum : int
{
    kClassGeneral = 0,
    kClassSingle = 1,
    kClassPairLow = 2,
    kClassPairHigh = 3
};
// where the kDirect instances write the rows they complete; no member, and nothing read, in the others
template <typename T, int kDirect>
struct LineDirect
{
    T *__restrict__ y;
};
template <typename T>
struct LineDirect<T, 0>
{
};
// kCoef (fdd_stiffness_matrix_lines_coef[_f32|_direct]): the factor arrays of a list whose unscaled blocks repeat, scaled by a
// coefficient per point, without streaming the scaled arrays.  Element e reads its three unscaled factor lines from block
// factor_elem[e] of three compact arrays (block c starts at c * 512; the lookup is wave-uniform and the loads are plain, as
// in kShared) and the coefficient at its own base, in each of the lane's three roles; g = coef * block is one IEEE double
// product, the statement the host made the scaled arrays with, rounded once to float in the float instance.  So the same
// words reach the same arithmetic as in the streamed instance on the scaled arrays.  coef and the blocks are double in both
// precisions; G is not read.  The lines are staged role by role -- the next role's two lines are requested before the
// current role's arithmetic and multiplied after it -- since all six raw lines at once do not fit beside the sums at
// four waves per SIMD.  No member, and nothing read, in the other instances
template <bool kCoef>
struct LineCoef
{
    const double *__restrict__ coef;
    const double *__restrict__ blk[3];
};
template <>
struct LineCoef<false>
{
};
// one role's raw lines, and their products
__device__ __forceinline__ void coef_line_load(double (&c)[8], double (&b)[8], const double *cp, const double *bp, int stride)
{
#pragma unroll
    for (int p = 0; p < 8; p++) c[p] = cp[stride * p];
#pragma unroll
    for (int p = 0; p < 8; p++) b[p] = bp[stride * p];
}
template <typename T>
__device__ __forceinline__ void coef_line_product(T (&g)[8], const double (&c)[8], const double (&b)[8])
{
#pragma unroll
    for (int p = 0; p < 8; p++) g[p] = (T)(c[p] * b[p]);
}

// the pair-low values of the workgroup's elements, by (j, k): LDS of the kDirect instances only
template <typename T>
__device__ __forceinline__ T *line_hand_over(int e_loc)
{
    __shared__ T s_h[LineCfg::epb][LineCfg::nn];
    return s_h[e_loc];
}

template <typename T, bool kGather, bool kNTStore, bool kShared = false, int kLean = 0, int kDirect = 0, bool kCoef = false>
__global__ __launch_bounds__(kBlock, 4) void line_stiffness_kernel_t(T *__restrict__ Au, const T *__restrict__ u, const int *__restrict__ point_dof, const double *__restrict__ u_scale, const T *__restrict__ D_hat, GPtrsT<T> G, const int *__restrict__ elem_offset, int num_elements, const int *__restrict__ factor_elem, LineDirect<T, kDirect> direct, LineCoef<kCoef> cf = {})
{
    static_assert(not(kCoef and kShared), "kCoef has its own way of addressing the shared blocks");
    using C = LineCfg;
    constexpr int n = C::n, nn = C::nn;
    static_assert(kDirect == 0 or kGather, "the classes of the points come with point_dof");
    __shared__ T s_a[C::epb][C::tile]; // u, then Au_2
    __shared__ T s_b[C::epb][C::tile]; // Au_1

    const int tid = threadIdx.x;
    const int e_loc = __builtin_amdgcn_readfirstlane(tid >> 6); // the wave is the element: bases stay in scalar registers
    const int l = tid & 63;
    const int a = l & 7, b = l >> 3;
    const int elem = blockIdx.x * C::epb + e_loc;
    if constexpr (kDirect == 0)
    {
        if (elem >= num_elements) return; // wave-uniform; nothing below waits for another wave
    }
    const bool active = kDirect == 0 or elem < num_elements; // kDirect: such a wave skips the element and goes to the barrier
    int d[n];                                                // the lane's entries of point_dof (kGather)
    T v[n];                                                  // its sums (kDirect: kept across the barrier)
    if (active)
    {
        const size_t base = elem_offset ? (size_t)elem_offset[elem] : (size_t)elem * C::n3;
        size_t fbase = base; // where the element's factor block is read
        if (kShared)
        {
            const int rep = factor_elem[elem];
            fbase = elem_offset ? (size_t)elem_offset[rep] : (size_t)rep * C::n3;
        }
        if (kCoef) fbase = (size_t)factor_elem[elem] * C::n3; // the compact arrays hold the distinct blocks one after another
        T *ta = s_a[e_loc], *tb = s_b[e_loc];
        constexpr bool kTerms = (kLean & kLeanTerms) != 0, kResident = (kLean & kLeanResident) != 0;
        static_assert(kTerms or not kResident, "the resident table does not hold the diagonal entries");
        const LeanTable<T, kResident> Dl(D_hat);

        // k-column role: u as in the slab form
        T r_u[n];
        if (kGather)
        {
            const int *pd = point_dof + base;
#pragma unroll
            for (int k = 0; k < n; k++) d[k] = __builtin_nontemporal_load(pd + (l + k * nn));
#pragma unroll
            for (int k = 0; k < n; k++) r_u[k] = u[d[k] < 0 ? 0 : (kDirect != 0 ? (d[k] & kDirectDofMask) : d[k])];
#pragma unroll
            for (int k = 0; k < n; k++) r_u[k] = (d[k] < 0) ? T(0) : r_u[k];
            if (u_scale)
            {
                const T sc = (T)(*u_scale);
#pragma unroll
                for (int k = 0; k < n; k++) r_u[k] = sc * r_u[k];
            }
        }
        else
        {
            const T *up = u + base;
#pragma unroll
            for (int k = 0; k < n; k++) r_u[k] = __builtin_nontemporal_load(up + (l + k * nn));
        }

        T r_3[n];
        if constexpr (not kTerms)
        {
#pragma unroll
            for (int m = 0; m < n; m++) r_3[m] = T(0);
        }

        {
            // the three factor lines of this lane, all requested before anything waits
            T g0[n], g1[n], g2[n];
            double cl[n], bl[n]; // kCoef: the raw lines of the role after the current one
            if constexpr (kCoef)
            {
                coef_line_load(cl, bl, cf.coef + base + l, cf.blk[2] + fbase + l, nn); // (i, j) = (a, b), k
                coef_line_product(g2, cl, bl);
                coef_line_load(cl, bl, cf.coef + base + 8 * l, cf.blk[0] + fbase + 8 * l, 1); // (j, k) = (a, b): the row
            }
            else
            {
#pragma unroll
                for (int k = 0; k < n; k++) g2[k] = kShared ? G.g[2][fbase + (l + k * nn)] : __builtin_nontemporal_load(G.g[2] + fbase + (l + k * nn)); // (i, j) = (a, b), k
                {
                    const T *g0p = G.g[0] + fbase + 8 * l; // (j, k) = (a, b): the row starts at 8 a + 64 b
#pragma unroll
                    for (int p = 0; p < n; p++) g0[p] = g0p[p];
                }
                {
                    const T *g1p = G.g[1] + fbase + (a + nn * b); // (i, k) = (a, b): the column steps by 8
#pragma unroll
                    for (int p = 0; p < n; p++) g1[p] = kShared ? g1p[8 * p] : __builtin_nontemporal_load(g1p + 8 * p);
                }
            }

#pragma unroll
            for (int k = 0; k < n; k++) ta[C::at(a, b, k)] = r_u[k];
            element_sync<true>();

            // z: registers only, Au_3(i, j, m) = sum_k D_hat[m + 8 k] * (g2_k * Du_3_k), k ascending
#pragma unroll
            for (int k = 0; k < n; k++)
            {
                if constexpr (kTerms)
                {
                    const T *Dk = Dl.row(k);
                    T Du_3 = Dl.at(Dk, k, 0) * r_u[0];
#pragma unroll
                    for (int p = 1; p < n; p++)
                        if (not lean_zero_entry(k, p)) Du_3 += Dl.at(Dk, k, p) * r_u[p];
                    const T GDu_3 = g2[k] * Du_3;
#pragma unroll
                    for (int m = 0; m < n; m++)
                    {
                        if (k == 0)
                            r_3[m] = Dl.at(Dk, 0, m) * GDu_3;
                        else if (not lean_zero_entry(k, m))
                            r_3[m] += Dl.at(Dk, k, m) * GDu_3;
                    }
                }
                else
                {
                    const T *Dk = line_row(D_hat, k);
                    T Du_3 = T(0);
#pragma unroll
                    for (int p = 0; p < n; p++) Du_3 += Dk[p] * r_u[p];
                    const T GDu_3 = g2[k] * Du_3;
#pragma unroll
                    for (int m = 0; m < n; m++) r_3[m] += Dk[m] * GDu_3;
                }
            }

            if constexpr (kCoef)
            {
                coef_line_product(g0, cl, bl);
                coef_line_load(cl, bl, cf.coef + base + (a + nn * b), cf.blk[1] + fbase + (a + nn * b), 8); // (i, k) = (a, b): the column
            }
            // x: the row out of the u tile, Au_1 into the other tile
            T ul[n], w[n], au[n];
#pragma unroll
            for (int p = 0; p < n; p++) ul[p] = ta[C::at(p, a, b)];
            if constexpr (kTerms) lean_du(w, ul, Dl); else line_du(w, ul, D_hat);
#pragma unroll
            for (int p = 0; p < n; p++) w[p] = g0[p] * w[p];
            if constexpr (kTerms) lean_au(au, w, Dl); else line_au(au, w, D_hat);
#pragma unroll
            for (int p = 0; p < n; p++) tb[C::at(p, a, b)] = au[p];
            // y: the column out of the u tile, Au_2 over it: every lane's row and column loads precede these stores in the
            // wave's instruction order, which the LDS keeps
#pragma unroll
            for (int p = 0; p < n; p++) ul[p] = ta[C::at(a, p, b)];
            element_sync<true>();
            if constexpr (kCoef) coef_line_product(g1, cl, bl);
            if constexpr (kTerms) lean_du(w, ul, Dl); else line_du(w, ul, D_hat);
#pragma unroll
            for (int p = 0; p < n; p++) w[p] = g1[p] * w[p];
            if constexpr (kTerms) lean_au(au, w, Dl); else line_au(au, w, D_hat);
#pragma unroll
            for (int p = 0; p < n; p++) ta[C::at(a, p, b)] = au[p];
            element_sync<true>();
        }

        T *Aup = Au + base;
        if constexpr (kDirect == 0)
        {
#pragma unroll
            for (int k = 0; k < n; k++)
            {
                v[k] = (tb[C::at(a, b, k)] + ta[C::at(a, b, k)]) + r_3[k];
                if (kNTStore)
                    __builtin_nontemporal_store(v[k], Aup + (l + k * nn));
                else
                    Aup[l + k * nn] = v[k];
            }
        }
        else
        {
#pragma unroll
            for (int k = 0; k < n; k++)
            {
                v[k] = (tb[C::at(a, b, k)] + ta[C::at(a, b, k)]) + r_3[k];
                const int cls = d[k] >> kDirectDofBits, dof = d[k] & kDirectDofMask; // a point without a dof: cls < 0
                if (cls == kClassGeneral)
                {
                    if (kNTStore)
                        __builtin_nontemporal_store(v[k], Aup + (l + k * nn));
                    else
                        Aup[l + k * nn] = v[k];
                }
                else if (cls == kClassSingle)
                {
                    const T s = T(0) + v[k];
                    if (kDirect == 2)
                        __builtin_nontemporal_store(s, direct.y + dof);
                    else
                        direct.y[dof] = s;
                }
                else if (cls == kClassPairLow)
                    line_hand_over<T>(e_loc)[b + 8 * k] = v[k];
            }
        }
    }
    if constexpr (kDirect != 0)
    {
        element_sync<false>(); // waits for the hand-over's LDS writes only: the stores above stay in flight
        if (active)
        {
            const T *left = line_hand_over<T>(e_loc > 0 ? e_loc - 1 : 0); // the classification never names wave 0 pair-high
#pragma unroll
            for (int k = 0; k < n; k++)
                if ((d[k] >> kDirectDofBits) == kClassPairHigh)
                {
                    const T s = (T(0) + left[b + 8 * k]) + v[k];
                    if (kDirect == 2)
                        __builtin_nontemporal_store(s, direct.y + (d[k] & kDirectDofMask));
                    else
                        direct.y[d[k] & kDirectDofMask] = s;
                }
        }
    }
}

// FDD_TUNE_ASSEMBLE_NT_STORE, read once: non-temporal stores of the rows of y the kDirect instances complete.  0: the next
// kernels read y (the multi-dot, the update), and non-temporal stores of such vectors measured slower before (HISTORY)
inline bool assemble_nt_store()
{
    static const bool nt_store = fdd_env_int("FDD_TUNE_ASSEMBLE_NT_STORE", 0) != 0;
    return nt_store;
}

// The one launcher of the degree-7 line kernel: which instance the run-time arguments name.
//   factor_elem given -> kShared -- never with kCoef, whose block_of_elem goes where factor_elem does and whose G is not read
//   direct_y given    -> kDirect 1 or 2 by assemble_nt_store(): double and gather only, which the dispatcher has checked
//   kLean, kCoef      -> the caller's; kDirectToo = false compiles no kDirect instance of this kLean
template <typename T, int kLean, bool kCoef, bool kDirectToo = true>
int launch_lines(T *Au, T *direct_y, const T *u, const int *point_dof, const double *u_scale, const T *D_hat, const GPtrsT<T> &G, const LineCoef<kCoef> &cf, const int *elem_offset, const int *factor_elem, int num_elements, void *stream)
{
    const int grid = (num_elements + LineCfg::epb - 1) / LineCfg::epb;
    auto launch = [&](auto gather, auto nt, auto shared, auto direct_kind) {
        constexpr int kDirect = decltype(direct_kind)::value;
        LineDirect<T, kDirect> direct;
        if constexpr (kDirect != 0) direct.y = direct_y;
        hipLaunchKernelGGL((line_stiffness_kernel_t<T, decltype(gather)::value, decltype(nt)::value, decltype(shared)::value, kLean, kDirect, kCoef>), dim3(grid), dim3(kBlock), 0, fdd_stream(stream), Au, u, point_dof, u_scale, D_hat, G, elem_offset, num_elements, factor_elem, direct, cf);
    };
    auto with_shared = [&](auto shared) {
        fdd_for_bool(stiffness_nt_store(), [&](auto nt) {
            if constexpr (sizeof(T) == 8 and kDirectToo)
                if (direct_y != nullptr)
                    return fdd_for_bool(assemble_nt_store(), [&](auto nt_y) { launch(std::true_type{}, nt, shared, std::integral_constant<int, decltype(nt_y)::value ? 2 : 1>{}); });
            fdd_for_bool(point_dof != nullptr, [&](auto gather) { launch(gather, nt, shared, std::integral_constant<int, 0>{}); });
        });
    };
    if constexpr (kCoef)
        with_shared(std::false_type{});
    else
        fdd_for_bool(factor_elem != nullptr, with_shared);
    FDD_LAUNCH_CHECK();
    return 0;
}

// A development build (-DFDD_LEAN_LINE_DEV) compiles both choices of the lean parts for both precisions and exports
// fdd_dev_lean_line_parts to choose between them at run time, for tools/lean_line_ab.py's per-part timings.
#ifdef FDD_LEAN_LINE_DEV
static int g_lean_line_parts = 0; // 0: the choice of the release build
extern "C" int fdd_dev_lean_line_parts(int parts)
{
    if (parts != 0 && parts != kLeanTerms && parts != (kLeanTerms | kLeanResident)) return FDD_ERR_UNSUPPORTED;
    g_lean_line_parts = parts;
    return 0;
}
#endif

// The entries of the line form; every refusal comes before the output is touched.
// streamed (fdd_stiffness_matrix_lines[_f32]): diag = 1: three factor arrays, G[3..5] are not passed on (never dereferenced).
//   diag = 0: six arrays -- that form was built and timed (see above), was not ahead of the slab form and is not compiled in
// shared (fdd_stiffness_matrix_lines_shared[_f32]): factor_elem names the element whose factor block each element reads;
//   three arrays only
// lean (fdd_stiffness_matrix_lines_lean[_f32]): the kLean instances, shared where factor_elem is given and streamed where it
//   is null; degree 7 on three arrays only.  The caller's guarantee about D_hat is in fdd_hip.h.  Double runs both parts,
//   float kLeanTerms (see above)
// coef (fdd_stiffness_matrix_lines_coef[_f32|_direct]): the kCoef instances, lean where the entry's `lean` says so; G is null,
//   cf holds the coefficient and the unscaled blocks, factor_elem is block_of_elem.  These entries refuse the degree first
//   and an empty list last, and an output may not be one of the inputs: not the same address, and where the elements lie one
//   after another (elem_offset null) no input may start inside the points Au covers.  The others allow Au == u
enum class LineEntry
{
    streamed,
    shared,
    lean,
    coef
};
// what the coefficient entries bring besides: the coefficient per point, the distinct unscaled blocks, and whether to run lean
struct LineCoefArgs
{
    const double *coef;
    const double *const *blocks;
    int lean;
};
// the coefficient entries' own checks of their pointers, in their order; block_of_elem goes where factor_elem does
template <typename T>
int lines_coef_check(const LineCoefArgs &ca, T *Au, T *direct_y, bool direct, const T *u, const int *point_dof, const double *u_scale, const T *D_hat, const int *block_of_elem, const int *elem_offset, int num_elements)
{
    FDD_REQUIRE(ca.coef != nullptr && ca.blocks != nullptr && ca.blocks[0] != nullptr && ca.blocks[1] != nullptr && ca.blocks[2] != nullptr && block_of_elem != nullptr);
    FDD_REQUIRE(Au != nullptr && u != nullptr && D_hat != nullptr);
    FDD_REQUIRE(not direct || (point_dof != nullptr && direct_y != nullptr));
    const char *lo = (const char *)Au, *hi = lo + (elem_offset ? sizeof(T) : (size_t)num_elements * LineCfg::n3 * sizeof(T));
    const void *inputs[] = {u, point_dof, u_scale, D_hat, ca.coef, ca.blocks[0], ca.blocks[1], ca.blocks[2], block_of_elem, elem_offset};
    for (const void *in : inputs)
    {
        const bool in_Au = (const char *)in >= lo && (const char *)in < hi;
        if (in != nullptr && (in_Au || (direct && in == (const void *)direct_y)))
        {
            fdd_set_error("the coefficient line form of the stiffness kernel: an output overlaps an input");
            return FDD_ERR_INVALID_ARGUMENT;
        }
    }
    if (direct && (const char *)direct_y >= lo && (const char *)direct_y < hi)
    {
        fdd_set_error("the coefficient line form of the stiffness kernel: y overlaps Au");
        return FDD_ERR_INVALID_ARGUMENT;
    }
    return 0;
}
// direct (fdd_stiffness_matrix_lines_direct, _coef_direct): the kDirect instance of the entry's kernel, which completes rows of
//   direct_y; double with point_dof only.  ca: the coefficient entries' and only theirs
template <typename T>
int lines_dispatch(LineEntry entry, T *Au, const T *u, const int *point_dof, const double *u_scale, const T *D_hat, const T *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, const int *factor_elem, int num_elements, int poly_degree, int diag, void *stream, bool direct = false, T *direct_y = nullptr, const LineCoefArgs &ca = {})
{
    static const char *const names[] = {"the line form", "the shared-block line form", "the lean line form", "the coefficient line form"};
    const bool coef = entry == LineEntry::coef;
    if (poly_degree != 7 && coef)
    {
        fdd_set_error("%s of the stiffness kernel supports poly_degree 7 only, got %d", names[(int)entry], poly_degree);
        return FDD_ERR_UNSUPPORTED;
    }
    if ((entry == LineEntry::shared || coef) && diag != 1)
    {
        fdd_set_error("%s of the stiffness kernel exists on three factor arrays only (diag = 1), got diag = %d", names[(int)entry], diag);
        return FDD_ERR_UNSUPPORTED;
    }
    FDD_REQUIRE(num_elements >= 0 && (entry == LineEntry::lean || diag == 0 || diag == 1));
    if (entry == LineEntry::lean && (poly_degree != 7 || diag != 1))
    {
        fdd_set_error("%s of the stiffness kernel supports poly_degree 7 on three factor arrays (diag = 1) only, got poly_degree %d, diag = %d", names[(int)entry], poly_degree, diag);
        return FDD_ERR_UNSUPPORTED;
    }
    if (poly_degree != 7)
    {
        fdd_set_error("%s of the stiffness kernel supports poly_degree 7 only, got %d", names[0], poly_degree);
        return FDD_ERR_UNSUPPORTED;
    }
    if (diag == 0)
    {
        fdd_set_error("the line form of the stiffness kernel on six factor arrays measured no faster than the slab form and is not compiled in (diag = 0)");
        return FDD_ERR_UNSUPPORTED;
    }
    GPtrsT<T> g{};
    if (coef)
    {
        if (int rc = lines_coef_check<T>(ca, Au, direct_y, direct, u, point_dof, u_scale, D_hat, factor_elem, elem_offset, num_elements)) return rc;
        if (num_elements == 0) return 0;
    }
    else
    {
        if (num_elements == 0) return 0;
        FDD_REQUIRE(Au != nullptr && u != nullptr && D_hat != nullptr && G != nullptr);
        FDD_REQUIRE(entry != LineEntry::shared || factor_elem != nullptr);
        FDD_REQUIRE(not direct || (point_dof != nullptr && direct_y != nullptr && (const void *)direct_y != (const void *)u && (const void *)direct_y != (const void *)Au));
        if (int rc = fdd_three_factors(g, G)) return rc;
    }
    const LineCoef<true> cf = coef ? LineCoef<true>{ca.coef, {ca.blocks[0], ca.blocks[1], ca.blocks[2]}} : LineCoef<true>{};
    T *y = direct ? direct_y : nullptr;
    constexpr int kParts = sizeof(T) == 8 ? (kLeanTerms | kLeanResident) : kLeanTerms; // the lean entries' parts
    if (coef && ca.lean != 0) return launch_lines<T, kParts, true>(Au, y, u, point_dof, u_scale, D_hat, g, cf, elem_offset, factor_elem, num_elements, stream);
    if (coef) return launch_lines<T, 0, true>(Au, y, u, point_dof, u_scale, D_hat, g, cf, elem_offset, factor_elem, num_elements, stream);
    if (entry != LineEntry::lean) return launch_lines<T, 0, false>(Au, y, u, point_dof, u_scale, D_hat, g, {}, elem_offset, entry == LineEntry::shared ? factor_elem : nullptr, num_elements, stream);
#ifdef FDD_LEAN_LINE_DEV
    constexpr int kOther = kParts ^ kLeanResident;
    if (y == nullptr && g_lean_line_parts == kOther) return launch_lines<T, kOther, false, false>(Au, y, u, point_dof, u_scale, D_hat, g, {}, elem_offset, factor_elem, num_elements, stream);
#endif
    return launch_lines<T, kParts, false>(Au, y, u, point_dof, u_scale, D_hat, g, {}, elem_offset, factor_elem, num_elements, stream);
}

// ---- factor blocks that repeat from element to element (the kShared line instance) ----
// One 64-bit hash per element over the bit patterns of its G[0..2] block.  Every word is mixed with its position in the
// block (array and point) through a bijection of 64-bit words and the results are added mod 2^64: two blocks that differ
// in one word differ in exactly one term and so in the hash, for certain; blocks that differ in more may collide, which
// is why fdd_stiffness_factor_block_verify has the last word.  The sum does not depend on the order of its terms.
__device__ __forceinline__ unsigned long long factor_word_mix(unsigned long long bits, unsigned long long position)
{
    unsigned long long z = bits + (position + 1ull) * 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(kBlock) void factor_block_hash_kernel(unsigned long long *__restrict__ out, GPtrs G, const int *__restrict__ elem_offset, int n3, int num_elements)
{
    __shared__ unsigned long long s_h[kBlock];
    for (int e = blockIdx.x; e < num_elements; e += gridDim.x) // block-uniform
    {
        const size_t base = elem_offset ? (size_t)elem_offset[e] : (size_t)e * n3;
        unsigned long long h = 0;
        for (int idx = threadIdx.x; idx < 3 * n3; idx += kBlock)
        {
            const int f = idx / n3;
            h += factor_word_mix((unsigned long long)__double_as_longlong(G.g[f][base + (idx - f * n3)]), (unsigned long long)idx);
        }
        s_h[threadIdx.x] = h;
        __syncthreads();
        for (int w = kBlock / 2; w > 0; w >>= 1)
        {
            if ((int)threadIdx.x < w) s_h[threadIdx.x] += s_h[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[e] = s_h[0];
        __syncthreads();
    }
}

// *mismatches += the number of elements whose block differs from the block of element factor_elem[e] in any bit of any of
// the three arrays (bits, not values: -0.0 is not 0.0, and NaN payloads count), or whose factor_elem[e] names no element.
// The entry clears mismatches before the launch.
__global__ __launch_bounds__(kBlock) void factor_block_verify_kernel(int *__restrict__ mismatches, GPtrs G, const int *__restrict__ elem_offset, const int *__restrict__ factor_elem, int n3, int num_elements)
{
    for (int e = blockIdx.x; e < num_elements; e += gridDim.x) // block-uniform
    {
        const int rep = factor_elem[e];
        int differs = 0;
        if (rep < 0 or rep >= num_elements)
            differs = 1;
        else if (rep != e)
        {
            const size_t base = elem_offset ? (size_t)elem_offset[e] : (size_t)e * n3;
            const size_t rbase = elem_offset ? (size_t)elem_offset[rep] : (size_t)rep * n3;
            for (int idx = threadIdx.x; idx < 3 * n3; idx += kBlock)
            {
                const int f = idx / n3;
                const int at = idx - f * n3;
                differs |= __double_as_longlong(G.g[f][base + at]) != __double_as_longlong(G.g[f][rbase + at]);
            }
        }
        if (__syncthreads_or(differs) and threadIdx.x == 0) atomicAdd(mismatches, 1);
    }
}

// flags[f] = 1 where array 3 + f of the list holds a value that is not a zero: any bit besides the sign set, so -0.0 passes
// and a denormal or a NaN does not, whatever the denormal mode.  flags are cleared by the caller; every lane that finds
// such a value stores the same 1.
__global__ __launch_bounds__(kBlock) void offdiag_zero_kernel(int *__restrict__ flags, GPtrs G, const int *__restrict__ elem_offset, int n3, size_t num_points)
{
    bool nz[3] = {false, false, false};
    for (size_t idx = (size_t)blockIdx.x * kBlock + threadIdx.x; idx < num_points; idx += (size_t)gridDim.x * kBlock)
    {
        const size_t e = idx / n3;
        const size_t at = elem_offset ? (size_t)elem_offset[e] + (idx - e * n3) : idx;
#pragma unroll
        for (int f = 0; f < 3; f++) nz[f] = nz[f] or (__double_as_longlong(G.g[3 + f][at]) & 0x7fffffffffffffffLL) != 0;
    }
#pragma unroll
    for (int f = 0; f < 3; f++)
        if (nz[f]) flags[f] = 1;
}

// One workgroup per element: c_f = G_f(p0) / W(p0) at the element's middle point, and the largest deviation of any
// factor of any point from c_f W(p), relative to max_f |c_f| W(p); W(p) = (w_i w_j) w_k as the kernel above forms it.
__global__ __launch_bounds__(kBlock) void affine_detect_kernel(double *__restrict__ c_out, double *__restrict__ deviation, GPtrs G, const int *__restrict__ elem_offset, const double *__restrict__ w, int n, int num_elements)
{
    __shared__ double s_c[FDD_NUM_GEOM_FACTS];
    __shared__ double s_max[kBlock / FDD_WAVE];
    const int e = blockIdx.x;
    if (e >= num_elements) return;
    const int n3 = n * n * n;
    const size_t base = elem_offset ? (size_t)elem_offset[e] : (size_t)e * n3;
    if (threadIdx.x < FDD_NUM_GEOM_FACTS)
    {
        const int m = n / 2, p0 = m + m * n + m * n * n;
        s_c[threadIdx.x] = G.g[threadIdx.x][base + p0] / ((w[m] * w[m]) * w[m]);
    }
    __syncthreads();
    double scale = 0.0;
#pragma unroll
    for (int f = 0; f < FDD_NUM_GEOM_FACTS; f++) scale = fmax(scale, fabs(s_c[f]));
    double worst = 0.0;
    for (int p = threadIdx.x; p < n3; p += kBlock)
    {
        const int i = p % n, j = (p / n) % n, k = p / (n * n);
        const double W = (w[i] * w[j]) * w[k];
#pragma unroll
        for (int f = 0; f < FDD_NUM_GEOM_FACTS; f++) worst = fmax(worst, fabs(G.g[f][base + p] - s_c[f] * W) / (scale * W));
    }
    if (!(scale > 0.0)) worst = 1.0; // all factors zero in the middle: not a usable element
#pragma unroll
    for (int off = FDD_WAVE / 2; off > 0; off >>= 1) worst = fmax(worst, __shfl_down(worst, off, FDD_WAVE));
    if ((threadIdx.x & (FDD_WAVE - 1)) == 0) s_max[threadIdx.x / FDD_WAVE] = worst;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        for (int v = 1; v < kBlock / FDD_WAVE; v++) worst = fmax(worst, s_max[v]);
        deviation[e] = worst;
#pragma unroll
        for (int f = 0; f < FDD_NUM_GEOM_FACTS; f++) c_out[(size_t)e * FDD_NUM_GEOM_FACTS + f] = s_c[f];
    }
}

template <typename T, int n>
int launch_fused_affine_t(T *Au, const T *u, const int *point_dof, const double *u_scale, const T *D_hat, const T *elem_factors, const T *gll_weights, const int *elem_offset, int num_elements, void *stream)
{
    using C = FusedCfg<n>;
    const int grid = (num_elements + C::epb - 1) / C::epb;
    GPtrsT<T> g;
    for (int k = 0; k < FDD_NUM_GEOM_FACTS; k++) g.g[k] = nullptr;
    g.g[0] = elem_factors;
    g.g[1] = gll_weights;
    fdd_for_bool(point_dof != nullptr, [&](auto gather) {
        hipLaunchKernelGGL((fused_stiffness_kernel_t<T, n, decltype(gather)::value, true, true>), dim3(grid), dim3(kBlock), 0, fdd_stream(stream), Au, u, point_dof, u_scale, D_hat, g, elem_offset, num_elements);
    });
    FDD_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int fused_dispatch_affine(T *Au, const T *u, const int *point_dof, const double *u_scale, const T *D_hat, const T *elem_factors, const T *gll_weights, const int *elem_offset, int num_elements, int poly_degree, void *stream)
{
    FDD_REQUIRE(num_elements >= 0);
    if (num_elements == 0) return 0;
    FDD_REQUIRE(Au != nullptr && u != nullptr && D_hat != nullptr && elem_factors != nullptr && gll_weights != nullptr);
    int rc = 0;
    if (fdd_for_n<2, 16>(poly_degree + 1, [&](auto n) { rc = launch_fused_affine_t<T, decltype(n)::value>(Au, u, point_dof, u_scale, D_hat, elem_factors, gll_weights, elem_offset, num_elements, stream); })) return rc;
    fdd_set_error("fused stiffness kernel supports poly_degree 1..15, got %d", poly_degree);
    return FDD_ERR_UNSUPPORTED;
}

// ---------------------------------------------------------------------------
// (2') fused kernel, 2-D, n = N+1 in [2, 16]: domain.okl:20-33 / :69-80 (the DIM == 2 branches)
// ---------------------------------------------------------------------------
// 40 B/point (u 8 + three geometric factors 24 + Au 8) against the two-launch form's 72.  One lane per point,
// floor(256 / n^2) elements per workgroup; the element and then G*Du go through LDS (rows padded by one double).
// Same operation order as the reference per point, so the result is bit-identical to the two-launch form.
template <int n, int kGroups, bool kNTStore>
__global__ __launch_bounds__(kBlock) void fused_stiffness_2d_kernel(double *__restrict__ Au, const double *__restrict__ u, const double *__restrict__ D_hat, GPtrs G, const int *__restrict__ elem_offset, int num_elements)
{
    constexpr int nn = n * n;
    constexpr int epb = kBlock / nn;
    constexpr int ld = n + 1;
    static_assert(epb >= 1, "an element must fit a workgroup");
    constexpr bool kWaveLocal = (64 % nn == 0); // an element never straddles a wavefront: no workgroup barrier between its LDS phases
    constexpr bool kDReg = (n <= 8);            // the four D_hat rows/columns of a lane in registers
    constexpr int nd = kDReg ? n : 1;

    __shared__ double s_D[nn];
    __shared__ double s_u[epb][n * ld];
    __shared__ double s_g[2][epb][n * ld];

    const int tid = threadIdx.x;
    const int e_loc = tid / nn;
    const int ij = tid - e_loc * nn;
    const int j = ij / n;
    const int i = ij - j * n;
    const int el = (e_loc < epb) ? e_loc : 0;
    const int lpos = i + j * ld;

    for (int t = tid; t < nn; t += kBlock) s_D[t] = D_hat[t];
    __syncthreads();
    double D_i[nd], D_j[nd], Dt_i[nd], Dt_j[nd];
    if (kDReg)
    {
#pragma unroll
        for (int k = 0; k < nd; k++)
        {
            D_i[k] = s_D[k + i * n];
            D_j[k] = s_D[k + j * n];
            Dt_i[k] = s_D[i + k * n];
            Dt_j[k] = s_D[j + k * n];
        }
    }

    // A workgroup takes kGroups consecutive groups of epb elements and requests all of their u and factors before it
    // computes the first: one point per lane and group is 32 B, too little in flight to cover the HBM latency.
    const int first = blockIdx.x * kGroups;
    bool active[kGroups];
    size_t at[kGroups];
    double r_u[kGroups], g0[kGroups], g1[kGroups], g2[kGroups];
#pragma unroll
    for (int q = 0; q < kGroups; q++)
    {
        const int elem = (first + q) * epb + e_loc;
        active[q] = (e_loc < epb) && (elem < num_elements);
        at[q] = 0;
        r_u[q] = g0[q] = g1[q] = g2[q] = 0.0;
        if (active[q])
        {
            at[q] = (elem_offset ? (size_t)elem_offset[elem] : (size_t)elem * nn) + ij;
            r_u[q] = __builtin_nontemporal_load(u + at[q]);
            g0[q] = __builtin_nontemporal_load(G.g[0] + at[q]);
            g1[q] = __builtin_nontemporal_load(G.g[1] + at[q]);
            g2[q] = __builtin_nontemporal_load(G.g[2] + at[q]);
        }
    }

    double *su = s_u[el];
    double *sg1 = s_g[0][el];
    double *sg2 = s_g[1][el];
#pragma unroll
    for (int q = 0; q < kGroups; q++)
    {
        if (active[q]) su[lpos] = r_u[q];
        element_sync<kWaveLocal>();

        int io = i, jo = j;
        if (!kDReg) asm volatile("" : "+v"(io), "+v"(jo));
        double Du_1 = 0.0, Du_2 = 0.0;
#pragma unroll
        for (int k = 0; k < n; k++)
        {
            const double di = kDReg ? D_i[kDReg ? k : 0] : s_D[k + io * n];
            const double dj = kDReg ? D_j[kDReg ? k : 0] : s_D[k + jo * n];
            Du_1 += di * su[k + j * ld];
            Du_2 += dj * su[i + k * ld];
        }
        if (active[q])
        {
            sg1[lpos] = g0[q] * Du_1 + g2[q] * Du_2;
            sg2[lpos] = g2[q] * Du_1 + g1[q] * Du_2;
        }
        element_sync<kWaveLocal>();

        double Au_1 = 0.0, Au_2 = 0.0;
#pragma unroll
        for (int k = 0; k < n; k++)
        {
            const double dti = kDReg ? Dt_i[kDReg ? k : 0] : s_D[io + k * n];
            const double dtj = kDReg ? Dt_j[kDReg ? k : 0] : s_D[jo + k * n];
            Au_1 += dti * sg1[k + j * ld];
            Au_2 += dtj * sg2[i + k * ld];
        }
        if (active[q])
        {
            if (kNTStore)
                __builtin_nontemporal_store(Au_1 + Au_2, Au + at[q]);
            else
                Au[at[q]] = Au_1 + Au_2;
        }
    }
}

template <int n>
int launch_fused_2d(double *Au, const double *u, const double *D_hat, const GPtrs &G, const int *elem_offset, int num_elements, void *stream)
{
    constexpr int epb = kBlock / (n * n);
    const int groups = (num_elements + epb - 1) / epb;
    static const int per_block = fdd_env_int("FDD_TUNE_STIFFNESS_2D_GROUPS", 4);
    auto launch = [&](auto per) {
        constexpr int K = decltype(per)::value;
        const int grid = (groups + K - 1) / K;
        fdd_for_bool(stiffness_nt_store(), [&](auto nt) {
            hipLaunchKernelGGL((fused_stiffness_2d_kernel<n, K, decltype(nt)::value>), dim3(grid), dim3(kBlock), 0, fdd_stream(stream), Au, u, D_hat, G, elem_offset, num_elements);
        });
    };
    // few elements: one group per workgroup keeps more workgroups in the launch
    if (per_block >= 4 && groups >= 4 * 2048)
        launch(std::integral_constant<int, 4>{});
    else if (per_block >= 2 && groups >= 2 * 2048)
        launch(std::integral_constant<int, 2>{});
    else
        launch(std::integral_constant<int, 1>{});
    FDD_LAUNCH_CHECK();
    return 0;
}

int fused_dispatch_2d(double *Au, const double *u, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream)
{
    FDD_REQUIRE(num_elements >= 0);
    if (num_elements == 0) return 0;
    FDD_REQUIRE(Au != nullptr && u != nullptr && D_hat != nullptr && G != nullptr);
    GPtrs g;
    for (int k = 0; k < FDD_NUM_GEOM_FACTS; k++) g.g[k] = G[k]; // 2-D reads G[0] = G11, G[1] = G22, G[2] = G12 only
    FDD_REQUIRE(g.g[0] != nullptr && g.g[1] != nullptr && g.g[2] != nullptr);
    int rc = 0;
    if (fdd_for_n<2, 16>(poly_degree + 1, [&](auto n) { rc = launch_fused_2d<decltype(n)::value>(Au, u, D_hat, g, elem_offset, num_elements, stream); })) return rc;
    fdd_set_error("fused 2-D stiffness kernel supports poly_degree 1..15, got %d (use the two-launch form)", poly_degree);
    return FDD_ERR_UNSUPPORTED;
}

int fill_level_table(LevelTable &T, const double *const *D_hat_ptr, const int *poly_degree, int num_levels)
{
    FDD_REQUIRE(D_hat_ptr != nullptr && poly_degree != nullptr && num_levels >= 1 && num_levels <= 16);
    for (int l = 0; l < 16; l++)
    {
        T.D_hat[l] = (l < num_levels) ? D_hat_ptr[l] : nullptr;
        T.poly_degree[l] = (l < num_levels) ? poly_degree[l] : 0;
    }
    return 0;
}

} // namespace

extern "C" {

int fdd_dom_stiffness_matrix_1(double *const GDu[3], const double *u, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], int num_points, int poly_degree, int dim, void *stream)
{
    FDD_REQUIRE(num_points >= 0 && poly_degree >= 1 && (dim == 2 || dim == 3));
    if (num_points == 0) return 0;
    FDD_REQUIRE(GDu != nullptr && u != nullptr && D_hat != nullptr && G != nullptr);
    GDuPtrs gd;
    GPtrs g;
    for (int k = 0; k < 3; k++) gd.g[k] = GDu[k];
    for (int k = 0; k < FDD_NUM_GEOM_FACTS; k++) g.g[k] = G[k];
    const int grid = (num_points + kBlock - 1) / kBlock;
    if (dim == 2)
        hipLaunchKernelGGL(dom_stiffness_1_kernel<2>, dim3(grid), dim3(kBlock), 0, fdd_stream(stream), gd, u, D_hat, g, num_points, poly_degree + 1);
    else
        hipLaunchKernelGGL(dom_stiffness_1_kernel<3>, dim3(grid), dim3(kBlock), 0, fdd_stream(stream), gd, u, D_hat, g, num_points, poly_degree + 1);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_dom_stiffness_matrix_2(double *Au, const double *const GDu[3], const double *D_hat, int num_points, int poly_degree, int dim, void *stream)
{
    FDD_REQUIRE(num_points >= 0 && poly_degree >= 1 && (dim == 2 || dim == 3));
    if (num_points == 0) return 0;
    FDD_REQUIRE(Au != nullptr && GDu != nullptr && D_hat != nullptr);
    GDuPtrs gd;
    for (int k = 0; k < 3; k++) gd.g[k] = const_cast<double *>(GDu[k]);
    const int grid = (num_points + kBlock - 1) / kBlock;
    if (dim == 2)
        hipLaunchKernelGGL(dom_stiffness_2_kernel<2>, dim3(grid), dim3(kBlock), 0, fdd_stream(stream), Au, gd, D_hat, num_points, poly_degree + 1);
    else
        hipLaunchKernelGGL(dom_stiffness_2_kernel<3>, dim3(grid), dim3(kBlock), 0, fdd_stream(stream), Au, gd, D_hat, num_points, poly_degree + 1);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_dom_stiffness_matrix(double *Au, const double *u, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], int num_elements, int poly_degree, void *stream)
{
    return fused_dispatch<double>(Au, u, nullptr, nullptr, D_hat, G, nullptr, num_elements, poly_degree, stream);
}

int fdd_sub_stiffness_matrix(double *Au, const double *u, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream)
{
    return fused_dispatch<double>(Au, u, nullptr, nullptr, D_hat, G, elem_offset, num_elements, poly_degree, stream);
}

int fdd_stiffness_matrix_2d(double *Au, const double *u, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream)
{
    return fused_dispatch_2d(Au, u, D_hat, G, elem_offset, num_elements, poly_degree, stream);
}

int fdd_sub_stiffness_matrix_gather(double *Au, const double *v, const int *point_dof, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream)
{
    FDD_REQUIRE(point_dof != nullptr);
    return fused_dispatch<double>(Au, v, point_dof, nullptr, D_hat, G, elem_offset, num_elements, poly_degree, stream);
}

int fdd_sub_stiffness_matrix_gather_scaled(double *Au, const double *v, const double *v_scale_dev, const int *point_dof, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream)
{
    FDD_REQUIRE(point_dof != nullptr);
    return fused_dispatch<double>(Au, v, point_dof, v_scale_dev, D_hat, G, elem_offset, num_elements, poly_degree, stream);
}

int fdd_stiffness_matrix_affine(double *Au, const double *v, const double *v_scale_dev, const int *point_dof, const double *D_hat, const double *elem_factors, const double *gll_weights, const int *elem_offset, int num_elements, int poly_degree, void *stream)
{
    return fused_dispatch_affine<double>(Au, v, point_dof, v_scale_dev, D_hat, elem_factors, gll_weights, elem_offset, num_elements, poly_degree, stream);
}

int fdd_stiffness_matrix_diag(double *Au, const double *v, const double *v_scale_dev, const int *point_dof, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream)
{
    return fused_dispatch<double, true>(Au, v, point_dof, v_scale_dev, D_hat, G, elem_offset, num_elements, poly_degree, stream);
}

int fdd_stiffness_matrix_diag_f32(float *Au, const float *v, const double *v_scale_dev, const int *point_dof, const float *D_hat, const float *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream)
{
    return fused_dispatch<float, true>(Au, v, point_dof, v_scale_dev, D_hat, G, elem_offset, num_elements, poly_degree, stream);
}

int fdd_stiffness_matrix_lines(double *Au, const double *v, const double *v_scale_dev, const int *point_dof, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, int diag, void *stream)
{
    return lines_dispatch<double>(LineEntry::streamed, Au, v, point_dof, v_scale_dev, D_hat, G, elem_offset, nullptr, num_elements, poly_degree, diag, stream);
}

int fdd_stiffness_matrix_lines_f32(float *Au, const float *v, const double *v_scale_dev, const int *point_dof, const float *D_hat, const float *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, int diag, void *stream)
{
    return lines_dispatch<float>(LineEntry::streamed, Au, v, point_dof, v_scale_dev, D_hat, G, elem_offset, nullptr, num_elements, poly_degree, diag, stream);
}

int fdd_stiffness_matrix_lines_direct(double *Au, double *y, const double *v, const double *v_scale_dev, const int *point_class_dof, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, const int *factor_elem, int lean, int num_elements, int poly_degree, int diag, void *stream)
{
    const LineEntry entry = lean != 0 ? LineEntry::lean : (factor_elem != nullptr ? LineEntry::shared : LineEntry::streamed);
    return lines_dispatch<double>(entry, Au, v, point_class_dof, v_scale_dev, D_hat, G, elem_offset, factor_elem, num_elements, poly_degree, diag, stream, true, y);
}

int fdd_stiffness_matrix_lines_shared(double *Au, const double *v, const double *v_scale_dev, const int *point_dof, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, const int *factor_elem, int num_elements, int poly_degree, int diag, void *stream)
{
    return lines_dispatch<double>(LineEntry::shared, Au, v, point_dof, v_scale_dev, D_hat, G, elem_offset, factor_elem, num_elements, poly_degree, diag, stream);
}

int fdd_stiffness_matrix_lines_shared_f32(float *Au, const float *v, const double *v_scale_dev, const int *point_dof, const float *D_hat, const float *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, const int *factor_elem, int num_elements, int poly_degree, int diag, void *stream)
{
    return lines_dispatch<float>(LineEntry::shared, Au, v, point_dof, v_scale_dev, D_hat, G, elem_offset, factor_elem, num_elements, poly_degree, diag, stream);
}

int fdd_stiffness_matrix_lines_lean(double *Au, const double *v, const double *v_scale_dev, const int *point_dof, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, const int *factor_elem, int num_elements, int poly_degree, int diag, void *stream)
{
    return lines_dispatch<double>(LineEntry::lean, Au, v, point_dof, v_scale_dev, D_hat, G, elem_offset, factor_elem, num_elements, poly_degree, diag, stream);
}

int fdd_stiffness_matrix_lines_lean_f32(float *Au, const float *v, const double *v_scale_dev, const int *point_dof, const float *D_hat, const float *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, const int *factor_elem, int num_elements, int poly_degree, int diag, void *stream)
{
    return lines_dispatch<float>(LineEntry::lean, Au, v, point_dof, v_scale_dev, D_hat, G, elem_offset, factor_elem, num_elements, poly_degree, diag, stream);
}

int fdd_stiffness_matrix_lines_coef(double *Au, const double *v, const double *v_scale_dev, const int *point_dof, const double *D_hat, const double *coef, const double *const blocks[3], const int *block_of_elem, const int *elem_offset, int lean, int num_elements, int poly_degree, int diag, void *stream)
{
    return lines_dispatch<double>(LineEntry::coef, Au, v, point_dof, v_scale_dev, D_hat, nullptr, elem_offset, block_of_elem, num_elements, poly_degree, diag, stream, false, nullptr, {coef, blocks, lean});
}

int fdd_stiffness_matrix_lines_coef_f32(float *Au, const float *v, const double *v_scale_dev, const int *point_dof, const float *D_hat, const double *coef, const double *const blocks[3], const int *block_of_elem, const int *elem_offset, int lean, int num_elements, int poly_degree, int diag, void *stream)
{
    return lines_dispatch<float>(LineEntry::coef, Au, v, point_dof, v_scale_dev, D_hat, nullptr, elem_offset, block_of_elem, num_elements, poly_degree, diag, stream, false, nullptr, {coef, blocks, lean});
}

int fdd_stiffness_matrix_lines_coef_direct(double *Au, double *y, const double *v, const double *v_scale_dev, const int *point_class_dof, const double *D_hat, const double *coef, const double *const blocks[3], const int *block_of_elem, const int *elem_offset, int lean, int num_elements, int poly_degree, int diag, void *stream)
{
    return lines_dispatch<double>(LineEntry::coef, Au, v, point_class_dof, v_scale_dev, D_hat, nullptr, elem_offset, block_of_elem, num_elements, poly_degree, diag, stream, true, y, {coef, blocks, lean});
}

constexpr int kFactorBlockGrid = 1 << 20; // workgroups; beyond it a workgroup takes several elements in turn
static int factor_block_args(GPtrs &g, const double *const G[FDD_NUM_GEOM_FACTS], int num_elements, int poly_degree)
{
    FDD_REQUIRE(num_elements >= 0 && poly_degree >= 1 && G != nullptr);
    if (poly_degree > 15)
    {
        fdd_set_error("the factor-block entries support poly_degree 1..15, got %d", poly_degree);
        return FDD_ERR_UNSUPPORTED;
    }
    return fdd_three_factors(g, G);
}

int fdd_stiffness_factor_block_hash(unsigned long long *out, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream)
{
    GPtrs g;
    if (int rc = factor_block_args(g, G, num_elements, poly_degree)) return rc;
    if (num_elements == 0) return 0;
    FDD_REQUIRE(out != nullptr);
    const int n = poly_degree + 1;
    hipLaunchKernelGGL(factor_block_hash_kernel, dim3(num_elements < kFactorBlockGrid ? num_elements : kFactorBlockGrid), dim3(kBlock), 0, fdd_stream(stream), out, g, elem_offset, n * n * n, num_elements);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_stiffness_factor_block_verify(int *mismatches, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, const int *factor_elem, int num_elements, int poly_degree, void *stream)
{
    GPtrs g;
    if (int rc = factor_block_args(g, G, num_elements, poly_degree)) return rc;
    FDD_REQUIRE(mismatches != nullptr);
    FDD_HIP_CHECK(hipMemsetAsync(mismatches, 0, sizeof(int), fdd_stream(stream)));
    if (num_elements == 0) return 0;
    FDD_REQUIRE(factor_elem != nullptr);
    const int n = poly_degree + 1;
    hipLaunchKernelGGL(factor_block_verify_kernel, dim3(num_elements < kFactorBlockGrid ? num_elements : kFactorBlockGrid), dim3(kBlock), 0, fdd_stream(stream), mismatches, g, elem_offset, factor_elem, n * n * n, num_elements);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_stiffness_offdiag_zero(int *flags_out, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream)
{
    FDD_REQUIRE(num_elements >= 0 && poly_degree >= 1 && flags_out != nullptr);
    FDD_HIP_CHECK(hipMemsetAsync(flags_out, 0, 3 * sizeof(int), fdd_stream(stream)));
    if (num_elements == 0) return 0;
    FDD_REQUIRE(G != nullptr && G[3] != nullptr && G[4] != nullptr && G[5] != nullptr);
    GPtrs g;
    for (int k = 0; k < FDD_NUM_GEOM_FACTS; k++) g.g[k] = G[k];
    const int n = poly_degree + 1, n3 = n * n * n;
    const size_t num_points = (size_t)num_elements * n3;
    hipLaunchKernelGGL(offdiag_zero_kernel, dim3(fdd_stream_grid((long long)num_points, kBlock)), dim3(kBlock), 0, fdd_stream(stream), flags_out, g, elem_offset, n3, num_points);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_stiffness_affine_detect(double *elem_factors, double *deviation, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, const double *gll_weights, int num_elements, int poly_degree, void *stream)
{
    FDD_REQUIRE(num_elements >= 0 && poly_degree >= 1);
    if (num_elements == 0) return 0;
    FDD_REQUIRE(elem_factors != nullptr && deviation != nullptr && G != nullptr && gll_weights != nullptr);
    GPtrs g;
    for (int k = 0; k < FDD_NUM_GEOM_FACTS; k++)
    {
        FDD_REQUIRE(G[k] != nullptr);
        g.g[k] = G[k];
    }
    hipLaunchKernelGGL(affine_detect_kernel, dim3(num_elements), dim3(kBlock), 0, fdd_stream(stream), elem_factors, deviation, g, elem_offset, gll_weights, poly_degree + 1, num_elements);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_stiffness_matrix_affine_f32(float *Au, const float *v, const double *v_scale_dev, const int *point_dof, const float *D_hat, const float *elem_factors, const float *gll_weights, const int *elem_offset, int num_elements, int poly_degree, void *stream)
{
    return fused_dispatch_affine<float>(Au, v, point_dof, v_scale_dev, D_hat, elem_factors, gll_weights, elem_offset, num_elements, poly_degree, stream);
}

int fdd_sub_stiffness_matrix_gather_scaled_f32(float *Au, const float *v, const double *v_scale_dev, const int *point_dof, const float *D_hat, const float *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream)
{
    FDD_REQUIRE(point_dof != nullptr);
    return fused_dispatch<float>(Au, v, point_dof, v_scale_dev, D_hat, G, elem_offset, num_elements, poly_degree, stream);
}

int fdd_sub_stiffness_matrix_1(double *const GDu[3], const double *u, const double *const *D_hat_ptr, const int *offset, const int *vert, const int *level, const int *poly_degree, int num_levels, const double *const G[FDD_NUM_GEOM_FACTS], int num_points, int dim, void *stream)
{
    FDD_REQUIRE(num_points >= 0 && (dim == 2 || dim == 3));
    if (num_points == 0) return 0;
    FDD_REQUIRE(GDu != nullptr && u != nullptr && offset != nullptr && vert != nullptr && level != nullptr && G != nullptr);
    LevelTable T;
    int rc = fill_level_table(T, D_hat_ptr, poly_degree, num_levels);
    if (rc) return rc;
    GDuPtrs gd;
    GPtrs g;
    for (int k = 0; k < 3; k++) gd.g[k] = GDu[k];
    for (int k = 0; k < FDD_NUM_GEOM_FACTS; k++) g.g[k] = G[k];
    const int grid = (num_points + kBlock - 1) / kBlock;
    if (dim == 2)
        hipLaunchKernelGGL(sub_stiffness_1_kernel<2>, dim3(grid), dim3(kBlock), 0, fdd_stream(stream), gd, u, T, offset, vert, level, g, num_points);
    else
        hipLaunchKernelGGL(sub_stiffness_1_kernel<3>, dim3(grid), dim3(kBlock), 0, fdd_stream(stream), gd, u, T, offset, vert, level, g, num_points);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_sub_stiffness_matrix_2(double *Au, const double *const GDu[3], const double *const *D_hat_ptr, const int *offset, const int *vert, const int *level, const int *poly_degree, int num_levels, int num_points, int dim, void *stream)
{
    FDD_REQUIRE(num_points >= 0 && (dim == 2 || dim == 3));
    if (num_points == 0) return 0;
    FDD_REQUIRE(Au != nullptr && GDu != nullptr && offset != nullptr && vert != nullptr && level != nullptr);
    LevelTable T;
    int rc = fill_level_table(T, D_hat_ptr, poly_degree, num_levels);
    if (rc) return rc;
    GDuPtrs gd;
    for (int k = 0; k < 3; k++) gd.g[k] = const_cast<double *>(GDu[k]);
    const int grid = (num_points + kBlock - 1) / kBlock;
    if (dim == 2)
        hipLaunchKernelGGL(sub_stiffness_2_kernel<2>, dim3(grid), dim3(kBlock), 0, fdd_stream(stream), Au, gd, T, offset, vert, level, num_points);
    else
        hipLaunchKernelGGL(sub_stiffness_2_kernel<3>, dim3(grid), dim3(kBlock), 0, fdd_stream(stream), Au, gd, T, offset, vert, level, num_points);
    FDD_LAUNCH_CHECK();
    return 0;
}

} // extern "C"
