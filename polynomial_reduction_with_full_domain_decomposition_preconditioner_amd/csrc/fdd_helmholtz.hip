// The zeroth-order term of a Helmholtz operator -laplace(u) + lambda u on assembled vectors (an addition of this build; the
// reference solves the Poisson problem only).  The SEM mass matrix is diagonal, so on a node or dof vector the term is a
// product with one precomputed vector c (host/domain.hpp, set_shift): y += c .* x behind the operator application that
// formed y, and, for the outer flexible CG, the same update with <x, y> of the values just stored -- the dot that follows
// the operator application there, which reads x and y anyway (16 B per element more than that dot: c read, y written;
// a pass of its own in front of it would move 32).
//
// HBM-bound, no reuse: the shapes are fdd_blas1.hip's (wide lanes where every pointer allows, a capped grid that strides)
// and fdd_reduce.hip's (private sums, a wavefront tree, one partial per workgroup in the common workspace, one final
// workgroup).  Compiled with -ffp-contract=off: y + c * x is a multiply and an add, in that order, at every width.
#include "fdd_stream.h"

namespace
{

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / FDD_WAVE;
constexpr int kEwMaxBlocks = 32768; // fdd_blas1.hip: element-wise kernels stream best with one access per lane

// y = y + c .* x, x standing for (*scale) * x where scale is given: the value the operator application in front was
// handed (an unnormalised Krylov vector and its 1/norm on the device; float vectors take the factor rounded to float, as
// fdd_vector_scaling_dev_f32 does).  Returns what it stored.
template <typename T>
struct ShiftAddOp
{
    T *y;
    const T *c, *x;
    const double *scale;
    template <typename A>
    __device__ __forceinline__ typename A::template value<T> at(A a, long long i) const
    {
        const auto yy = a.ld(y, i), cc = a.ld(c, i);
        auto xx = a.ld(x, i);
        if (scale) xx = (T)(*scale) * xx;
        const auto v = yy + cc * xx;
        a.st(y, i, v);
        return v;
    }
    template <typename F>
    void pointers(F f) const { f(y), f(c), f(x); }
};

// nw lane elements of W values each, then the values behind the last whole one (nw = 0: every value, one per lane)
template <typename T, int W>
__global__ __launch_bounds__(kBlock) void shift_add_kernel(ShiftAddOp<T> op, long long nw, long long n)
{
    const long long stride = (long long)gridDim.x * kBlock;
    const long long first = (long long)blockIdx.x * kBlock + threadIdx.x;
    for (long long i = first; i < nw; i += stride) op.at(fdd_lanes<W>{}, i);
    for (long long i = W * nw + first; i < n; i += stride) op.at(fdd_lanes<1>{}, i);
}

// the same update and, of the values it stores, sum x * y: Dot2Op's term (fdd_reduce.hip) with y not read back
template <int W>
__global__ __launch_bounds__(kBlock) void shift_add_dot_kernel(ShiftAddOp<double> op, double *ws, long long nw, long long n)
{
    double sum = 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    const long long first = (long long)blockIdx.x * kBlock + threadIdx.x;
    for (long long i = first; i < nw; i += stride)
    {
        const fdd_lanes<W> l{};
        const auto xx = l.ld(op.x, i); // before the store: nothing here lets the compiler know that y is not x
        l.add(sum, xx * op.at(l, i));
    }
    for (long long i = W * nw + first; i < n; i += stride)
    {
        const double xx = op.x[i];
        sum += xx * op.at(fdd_lanes<1>{}, i);
    }

    // fdd_reduce.hip's block_reduce_store and reduce_final_kernel for one value
    __shared__ double s[kWaves];
    const int lane = threadIdx.x & (FDD_WAVE - 1), wave = threadIdx.x / FDD_WAVE;
    const double x = wave_sum(sum);
    if (lane == 0) s[wave] = x;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        double t = s[0];
#pragma unroll
        for (int w = 1; w < kWaves; w++) t += s[w];
        ws[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(kBlock) void shift_add_dot_final_kernel(double *out, const double *ws, int nblocks)
{
    __shared__ double s[kWaves];
    const int lane = threadIdx.x & (FDD_WAVE - 1), wave = threadIdx.x / FDD_WAVE;
    double x = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += kBlock) x += ws[b];
    x = wave_sum(x);
    if (lane == 0) s[wave] = x;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        double t = s[0];
#pragma unroll
        for (int w = 1; w < kWaves; w++) t += s[w];
        out[0] = t;
    }
}

template <typename T>
bool overlap(const T *a, const T *b, long long n)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b), bytes = (uintptr_t)n * sizeof(T);
    return a0 < b0 + bytes && b0 < a0 + bytes;
}

// the lane elements of the wide path: W values in 16 bytes where every pointer is 16-byte aligned, else none
template <typename T>
long long wide_count(const ShiftAddOp<T> &op, long long n)
{
    constexpr int W = 16 / (int)sizeof(T);
    return fdd_lanes_fit<fdd_lanes<W>>(op) ? n / W : 0;
}

template <typename T>
int shift_add(T *y, const T *c, const double *scale_dev, const T *x, int n, void *stream)
{
    FDD_REQUIRE(n >= 0);
    if (n == 0) return 0;
    FDD_REQUIRE(y != nullptr && c != nullptr && x != nullptr);
    FDD_REQUIRE(!overlap(y, c, n) && !overlap(y, x, n));
    constexpr int W = 16 / (int)sizeof(T);
    const ShiftAddOp<T> op{y, c, x, scale_dev};
    const long long nw = wide_count(op, n);
    hipLaunchKernelGGL((shift_add_kernel<T, W>), dim3(fdd_stream_grid(nw > 0 ? nw : n, kBlock, kEwMaxBlocks)), dim3(kBlock), 0, fdd_stream(stream), op, nw, (long long)n);
    FDD_LAUNCH_CHECK();
    return 0;
}

// The same statement on the support of c alone, for a c that is zero on most of the vector (a Robin term lives on the
// boundary nodes): entry k of the compressed values belongs to element index[k].  The indices are distinct and ascending,
// so no two lanes meet and nothing but y[index[k]] is written; one entry per lane -- its three accesses are scattered, there
// is nothing to widen.  An index outside 0..n-1 (the host layer builds the list; a caller's mistake) is skipped, not followed.
template <typename T>
__global__ __launch_bounds__(kBlock) void shift_add_indexed_kernel(T *__restrict__ y, const T *__restrict__ c_values, const int *__restrict__ index, long long m, const double *scale, const T *__restrict__ x, int n)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long k = (long long)blockIdx.x * kBlock + threadIdx.x; k < m; k += stride)
    {
        const int i = index[k];
        if (i < 0 || i >= n) continue;
        T xx = x[i];
        if (scale) xx = (T)(*scale) * xx;
        y[i] = y[i] + c_values[k] * xx;
    }
}

template <typename T>
int shift_add_indexed(T *y, const T *c_values, const int *index, int m, const double *scale_dev, const T *x, int n, void *stream)
{
    FDD_REQUIRE(n >= 0 && m >= 0 && m <= n);
    if (m == 0) return 0;
    FDD_REQUIRE(y != nullptr && c_values != nullptr && index != nullptr && x != nullptr);
    FDD_REQUIRE(!overlap(y, x, n));
    const uintptr_t y0 = reinterpret_cast<uintptr_t>(y), y1 = y0 + (uintptr_t)n * sizeof(T);
    const uintptr_t c0 = reinterpret_cast<uintptr_t>(c_values), i0 = reinterpret_cast<uintptr_t>(index);
    FDD_REQUIRE(!(y0 < c0 + (uintptr_t)m * sizeof(T) && c0 < y1));
    FDD_REQUIRE(!(y0 < i0 + (uintptr_t)m * sizeof(int) && i0 < y1));
    hipLaunchKernelGGL((shift_add_indexed_kernel<T>), dim3(fdd_stream_grid(m, kBlock, kEwMaxBlocks)), dim3(kBlock), 0, fdd_stream(stream), y, c_values, index, (long long)m, scale_dev, x, n);
    FDD_LAUNCH_CHECK();
    return 0;
}

} // namespace

extern "C" {

int fdd_shift_add_indexed(double *y, const double *c_values, const int *index, int m, const double *scale_dev, const double *x, int n, void *stream) { return shift_add_indexed(y, c_values, index, m, scale_dev, x, n, stream); }

int fdd_shift_add_indexed_f32(float *y, const float *c_values, const int *index, int m, const double *scale_dev, const float *x, int n, void *stream) { return shift_add_indexed(y, c_values, index, m, scale_dev, x, n, stream); }

int fdd_shift_add(double *y, const double *c, const double *scale_dev, const double *x, int n, void *stream) { return shift_add(y, c, scale_dev, x, n, stream); }

int fdd_shift_add_f32(float *y, const float *c, const double *scale_dev, const float *x, int n, void *stream) { return shift_add(y, c, scale_dev, x, n, stream); }

int fdd_shift_add_inner_product(double *out, double *ws, double *y, const double *c, const double *x, int n, void *stream)
{
    FDD_REQUIRE(out != nullptr && ws != nullptr && n >= 0);
    hipStream_t s = fdd_stream(stream);
    if (n == 0) return (int)hipMemsetAsync(out, 0, sizeof(double), s); // an empty sum is zero, as in every reduction entry
    FDD_REQUIRE(y != nullptr && c != nullptr && x != nullptr);
    FDD_REQUIRE(!overlap<double>(y, c, n) && !overlap<double>(y, x, n));
    const ShiftAddOp<double> op{y, c, x, nullptr};
    const long long nw = wide_count(op, n);
    const int grid = fdd_stream_grid(nw > 0 ? nw : n, kBlock);
    hipLaunchKernelGGL(shift_add_dot_kernel<2>, dim3(grid), dim3(kBlock), 0, s, op, ws, nw, (long long)n);
    FDD_LAUNCH_CHECK();
    hipLaunchKernelGGL(shift_add_dot_final_kernel, dim3(1), dim3(kBlock), 0, s, out, ws, grid);
    FDD_LAUNCH_CHECK();
    return 0;
}

} // extern "C"
