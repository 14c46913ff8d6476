// Setup of the low-order AMG hierarchy on the device (include/fdd_hip.h, "AMG setup").
//
// Every kernel restates one routine of host/low_order.hpp operation for operation, so that a hierarchy built here is
// the host's bit for bit (the build is -ffp-contract=off: multiply, then add, as g++ -O2 does on x86-64):
//   fem_stencils / fem_count / fem_fill   low_order::assemble_fem + from_triplets
//   spgemm_count / spgemm_fill            low_order::multiply (Gustavson)
//   transpose_count / transpose_fill      low_order::transpose (drop_tol < 0) and CSR_Matrix::transpose (drop_tol >= 0)
//   inv_sqrt_diagonal                     diagonal() and D = 1 / sqrt(d) of low_order::build
//   lattice_*                             low_order::geometric_level on a conforming lattice (interpolator, coarse lattice, Transfer maps)
// Sparse results are built count -> row pointers -> fill; the row pointers are scanned on the host in 64-bit arithmetic
// (fdd_amg_setup_row_pointers), which is where an int overflow of the entry count is caught.
#include <climits>
#include <vector>

#include "fdd_common.h"

namespace
{

constexpr int kBlock = 256;

inline int blocks_for(long long n) { return (int)((n + kBlock - 1) / kBlock); }

// ---------------------------------------------------------------------------------------------------------------
// C = A * B.  One lane per row of C.  The rows of B named by A's row are sorted by column, so C's row in ascending
// column order is their k-way merge: a cursor per entry of A's row (kept in the caller's workspace at the entry's own
// index) and, per output column j, one pass over A's row in order adding a_ik * b_kj where the cursor of k sits on j.
// acc[j] of the host's Gustavson loop takes exactly these products in exactly this order (A's row, then B's row),
// starting from 0.0.
// ---------------------------------------------------------------------------------------------------------------
template <bool FILL>
__global__ void spgemm_kernel(int *__restrict__ row_len, int *__restrict__ C_col, double *__restrict__ C_val, int *__restrict__ cursor, const int *__restrict__ C_ptr,
                              const int *__restrict__ A_ptr, const int *__restrict__ A_col, const double *__restrict__ A_val, const int *__restrict__ B_ptr, const int *__restrict__ B_col,
                              const double *__restrict__ B_val, int a_rows, int b_rows)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a_rows) return;
    const int p0 = A_ptr[i], p1 = A_ptr[i + 1];
    for (int p = p0; p < p1; p++)
    {
        const int k = A_col[p];
        cursor[p] = (k >= 0 and k < b_rows) ? B_ptr[k] : 0;
    }
    int out = FILL ? C_ptr[i] : 0;
    const int out_end = FILL ? C_ptr[i + 1] : INT_MAX;
    int count = 0;
    while (true)
    {
        int j = INT_MAX;
        for (int p = p0; p < p1; p++)
        {
            const int k = A_col[p];
            if (k < 0 or k >= b_rows) continue;
            const int q = cursor[p];
            if (q < B_ptr[k + 1] and B_col[q] < j) j = B_col[q];
        }
        if (j == INT_MAX) break;
        double s = 0.0;
        for (int p = p0; p < p1; p++)
        {
            const int k = A_col[p];
            if (k < 0 or k >= b_rows) continue;
            int q = cursor[p];
            const int q1 = B_ptr[k + 1];
            if (q >= q1 or B_col[q] != j) continue;
            const double a = A_val ? A_val[p] : 0.0;
            for (; q < q1 and B_col[q] == j; q++)
                if (FILL) s += a * B_val[q];
            cursor[p] = q;
        }
        if (FILL)
        {
            if (out >= out_end) return; // the row pointers do not belong to these matrices: write nothing past the row
            C_col[out] = j;
            C_val[out] = s;
            out++;
        }
        count++;
    }
    if (not FILL) row_len[i] = count;
}

// ---------------------------------------------------------------------------------------------------------------
// T = A^T.  Entries are counted per column with integer atomics, placed at atomically taken slots of their column
// (their source index only), and every row of T is then sorted by source index: ascending source index is A's row
// order, i.e. the counting sort's stable order.  Values only move.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool kept_entry(const double *A_val, int p, double drop_tol) { return drop_tol < 0.0 or A_val == nullptr or fabs(A_val[p]) > drop_tol; }

__global__ void transpose_count_kernel(int *__restrict__ row_len, const int *__restrict__ A_ptr, const int *__restrict__ A_col, const double *__restrict__ A_val, int a_rows, int a_cols, double drop_tol)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a_rows) return;
    for (int p = A_ptr[i]; p < A_ptr[i + 1]; p++)
    {
        const int c = A_col[p];
        if (c >= 0 and c < a_cols and kept_entry(A_val, p, drop_tol)) atomicAdd(&row_len[c], 1);
    }
}

__global__ void transpose_place_kernel(int *__restrict__ src, int *__restrict__ cursor, const int *__restrict__ A_ptr, const int *__restrict__ A_col, const double *__restrict__ A_val, int a_rows, int a_cols, double drop_tol,
                                       int nnz_t)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a_rows) return;
    for (int p = A_ptr[i]; p < A_ptr[i + 1]; p++)
    {
        const int c = A_col[p];
        if (c < 0 or c >= a_cols or not kept_entry(A_val, p, drop_tol)) continue;
        const int slot = atomicAdd(&cursor[c], 1);
        if (slot < nnz_t) src[slot] = p;
    }
}

__global__ void transpose_order_kernel(int *__restrict__ T_col, double *__restrict__ T_val, int *__restrict__ src, const int *__restrict__ T_ptr, const int *__restrict__ A_ptr, const double *__restrict__ A_val, int a_rows, int t_rows)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= t_rows) return;
    const int q0 = T_ptr[r], q1 = T_ptr[r + 1];
    for (int q = q0 + 1; q < q1; q++) // insertion sort: the rows are short (a column of an interpolator or of a lattice map)
    {
        const int v = src[q];
        int w = q - 1;
        for (; w >= q0 and src[w] > v; w--) src[w + 1] = src[w];
        src[w + 1] = v;
    }
    for (int q = q0; q < q1; q++)
    {
        const int p = src[q];
        int lo = 0, hi = a_rows; // the row of entry p: the last i with A_ptr[i] <= p
        while (hi - lo > 1)
        {
            const int mid = lo + (hi - lo) / 2;
            if (A_ptr[mid] <= p)
                lo = mid;
            else
                hi = mid;
        }
        T_col[q] = lo;
        if (T_val) T_val[q] = A_val[p];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Low-order FEM rows.  Stencil: one lane per element point sums, over the cells of its element that touch it in the
// host's order (sz, sy, sx, t), the entries of its own row of every tetrahedron with the point as a vertex, into the
// 27 slots of its neighbours -- the host's K / touched for this point's row, same additions in the same order.
// ---------------------------------------------------------------------------------------------------------------
__constant__ int c_tets[6][4][3] = {{{0, 0, 0}, {0, 1, 0}, {1, 0, 0}, {1, 0, 1}}, {{1, 0, 0}, {0, 1, 0}, {1, 1, 0}, {1, 0, 1}}, {{0, 0, 0}, {0, 0, 1}, {0, 1, 0}, {1, 0, 1}},
                                    {{1, 0, 1}, {1, 1, 0}, {1, 1, 1}, {0, 1, 0}}, {{0, 0, 1}, {1, 0, 1}, {0, 1, 1}, {0, 1, 0}}, {{1, 0, 1}, {1, 1, 1}, {0, 1, 1}, {0, 1, 0}}};

__global__ void fem_stencil_kernel(double *__restrict__ K, unsigned int *__restrict__ mask, const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z, const int *__restrict__ point_dof,
                                   int N, long long num_points, double epsilon)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= num_points) return;
    const int n = N + 1, n3 = n * n * n;
    const long long base = (g / n3) * n3;
    const int li = (int)(g - base);
    const int px = li % n, py = (li / n) % n, pz = li / (n * n);
    double Ks[27];
    unsigned int touched = 0;
#pragma unroll
    for (int s = 0; s < 27; s++) Ks[s] = 0.0;
    if (point_dof[g] >= 0)
        for (int sz = (pz > 0 ? pz - 1 : 0); sz <= (pz < N ? pz : N - 1); sz++)
            for (int sy = (py > 0 ? py - 1 : 0); sy <= (py < N ? py : N - 1); sy++)
                for (int sx = (px > 0 ? px - 1 : 0); sx <= (px < N ? px : N - 1); sx++)
                    for (int t = 0; t < 6; t++)
                    {
                        int i = -1;
                        for (int v = 0; v < 4; v++)
                            if (sx + c_tets[t][v][0] == px and sy + c_tets[t][v][1] == py and sz + c_tets[t][v][2] == pz) i = v;
                        if (i < 0) continue;
                        long long loc[4];
                        double xs[4], ys[4], zs[4];
                        for (int v = 0; v < 4; v++)
                        {
                            loc[v] = base + (sx + c_tets[t][v][0]) + (long long)(sy + c_tets[t][v][1]) * n + (long long)(sz + c_tets[t][v][2]) * n * n;
                            xs[v] = x[loc[v]];
                            ys[v] = y[loc[v]];
                            zs[v] = z[loc[v]];
                        }
                        const double H[9] = {xs[0] - xs[3], xs[1] - xs[3], xs[2] - xs[3], ys[0] - ys[3], ys[1] - ys[3], ys[2] - ys[3], zs[0] - zs[3], zs[1] - zs[3], zs[2] - zs[3]};
                        const double det = H[0] * (H[4] * H[8] - H[5] * H[7]) - H[1] * (H[3] * H[8] - H[5] * H[6]) + H[2] * (H[3] * H[7] - H[4] * H[6]);
                        const double id = 1.0 / det;
                        const double iH[9] = {id * (H[4] * H[8] - H[7] * H[5]), id * (H[2] * H[7] - H[8] * H[1]), id * (H[1] * H[5] - H[4] * H[2]),
                                              id * (H[5] * H[6] - H[8] * H[3]), id * (H[0] * H[8] - H[6] * H[2]), id * (H[2] * H[3] - H[5] * H[0]),
                                              id * (H[3] * H[7] - H[6] * H[4]), id * (H[1] * H[6] - H[7] * H[0]), id * (H[0] * H[4] - H[3] * H[1])};
                        double G[3][3];
                        for (int m = 0; m < 3; m++)
                            for (int nn = 0; nn < 3; nn++)
                            {
                                double gs = 0.0;
                                for (int k = 0; k < 3; k++) gs += (det / 24.0) * iH[m * 3 + k] * iH[nn * 3 + k];
                                G[m][nn] = gs;
                            }
                        for (int j = 0; j < 4; j++)
                        {
                            double a = 0.0;
                            const int m0 = (i < 3) ? i : 0, m1 = (i < 3) ? i + 1 : 3, n0 = (j < 3) ? j : 0, n1 = (j < 3) ? j + 1 : 3;
                            const bool minus = (i < 3) != (j < 3);
                            for (int m = m0; m < m1; m++)
                                for (int nn = n0; nn < n1; nn++)
                                {
                                    const double gv = minus ? -G[m][nn] : G[m][nn];
                                    for (int q = 0; q < 4; q++) a += gv;
                                }
                            if (point_dof[loc[j]] < 0 or not(fabs(a) > epsilon)) continue;
                            const int d0 = c_tets[t][j][0] - c_tets[t][i][0], d1 = c_tets[t][j][1] - c_tets[t][i][1], d2 = c_tets[t][j][2] - c_tets[t][i][2];
                            const int slot = (d0 + 1) + 3 * (d1 + 1) + 9 * (d2 + 1);
                            Ks[slot] += a;
                            touched |= 1u << slot;
                        }
                    }
    for (int s = 0; s < 27; s++) K[(size_t)g * 27 + s] = Ks[s];
    mask[g] = touched;
}

// One lane per dof: the entries of its occurrences (ascending points, slots in order) are the host's triplets of this
// row in arrival order; from_triplets sorts them stably by column and sums equal columns from the first one on.
template <bool FILL>
__global__ void fem_row_kernel(int *__restrict__ row_len, int *__restrict__ A_col, double *__restrict__ A_val, const int *__restrict__ A_ptr, const int *__restrict__ dof_ptr, const int *__restrict__ dof_points,
                               const unsigned int *__restrict__ mask, const double *__restrict__ K, const int *__restrict__ point_dof, int N, int num_dofs)
{
    const long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= num_dofs) return;
    const int n = N + 1;
    const int o0 = dof_ptr[d], o1 = dof_ptr[d + 1];
    int out = FILL ? A_ptr[d] : 0;
    const int out_end = FILL ? A_ptr[d + 1] : INT_MAX;
    int count = 0, last = -1;
    while (true)
    {
        int j = INT_MAX;
        for (int o = o0; o < o1; o++)
        {
            const long long g = dof_points[o];
            unsigned int m = mask[g];
            while (m)
            {
                const int s = __ffs(m) - 1;
                m &= m - 1;
                const int c = point_dof[g + (s % 3 - 1) + ((s / 3) % 3 - 1) * n + (s / 9 - 1) * n * n];
                if (c > last and c < j) j = c;
            }
        }
        if (j == INT_MAX) break;
        if (FILL)
        {
            double v = 0.0;
            bool first = true;
            for (int o = o0; o < o1; o++)
            {
                const long long g = dof_points[o];
                unsigned int m = mask[g];
                while (m)
                {
                    const int s = __ffs(m) - 1;
                    m &= m - 1;
                    if (point_dof[g + (s % 3 - 1) + ((s / 3) % 3 - 1) * n + (s / 9 - 1) * n * n] != j) continue;
                    const double k = K[(size_t)g * 27 + s];
                    if (first)
                        v = k;
                    else
                        v += k;
                    first = false;
                }
            }
            if (out >= out_end) return;
            A_col[out] = j;
            A_val[out] = v;
            out++;
        }
        count++;
        last = j;
    }
    if (not FILL) row_len[d] = count;
}

__global__ void inv_sqrt_diagonal_kernel(double *__restrict__ D, const int *__restrict__ A_ptr, const int *__restrict__ A_col, const double *__restrict__ A_val, int rows)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    double d = 0.0;
    for (int p = A_ptr[i]; p < A_ptr[i + 1]; p++)
        if (A_col[p] == i) d = A_val[p];
    D[i] = 1.0 / sqrt(d);
}

__global__ void unit_values_kernel(int *__restrict__ flag, const double *__restrict__ val, long long nnz)
{
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += (long long)gridDim.x * blockDim.x)
        if (val[p] != 1.0) flag[0] = 0; // every lane that writes writes the same value
}

// ---------------------------------------------------------------------------------------------------------------
// One geometric level (low_order::geometric_level) on a conforming 3-D lattice, where every lattice point carries
// one dof with a unit entry or none: the lattice is its point -> dof array (-1: no dof).  The 1-D tables (kept nodes,
// lo / hi / wl of every node) are small and come from the host.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kMaxNodes = 32;
struct LatticeTables
{
    int n, m;
    int keep[kMaxNodes], lo[kMaxNodes], hi[kMaxNodes], pos[kMaxNodes];
    double wl[kMaxNodes];
};

// first[d]: the first point of dof d (the serial scan's); kept[d]: some point of d is a kept node in every direction
__global__ void lattice_first_kernel(int *__restrict__ first, int *__restrict__ kept, const int *__restrict__ point_dof, long long num_points, int num_dofs, LatticeTables t)
{
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= num_points) return;
    const int d = point_dof[q];
    if (d < 0 or d >= num_dofs) return;
    const int n = t.n;
    const long long v = q % ((long long)n * n * n);
    atomicMin(&first[d], (int)q);
    if (t.pos[v % n] >= 0 and t.pos[(v / n) % n] >= 0 and t.pos[v / (n * n)] >= 0) kept[d] = 1; // every writer writes 1
}

__global__ void lattice_coarse_flag_kernel(int *__restrict__ flag, const int *__restrict__ first, const int *__restrict__ kept, int num_dofs)
{
    const long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= num_dofs) return;
    flag[d] = (first[d] == INT_MAX or kept[d]) ? 1 : 0;
}

// cmap[d] = the coarse dof of a kept dof (cstart: exclusive prefix count of the flags), -1 otherwise; owner_dof[first[d]] = d
__global__ void lattice_cmap_kernel(int *__restrict__ cmap, int *__restrict__ owner_dof, int *__restrict__ unplaced, const int *__restrict__ cstart, const int *__restrict__ first, const int *__restrict__ kept, int num_dofs)
{
    const long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= num_dofs) return;
    const bool none = first[d] == INT_MAX;
    cmap[d] = (none or kept[d]) ? cstart[d] : -1;
    if (none)
        unplaced[0] = 1; // a dof on no lattice point: the interpolator is not the plain lattice interpolation
    else
        owner_dof[first[d]] = (int)d;
}

// the P row of dof d: one unit entry for a kept dof; else the multi-linear weights of the up to 8 kept corners around its
// first point, sorted by coarse column (stable, as std::sort is on rows this short) with equal columns summed in order
template <bool FILL>
__global__ void lattice_interp_kernel(int *__restrict__ row_len, int *__restrict__ P_col, double *__restrict__ P_val, const int *__restrict__ P_ptr, const int *__restrict__ cmap, const int *__restrict__ first,
                                      const int *__restrict__ point_dof, int num_dofs, LatticeTables t)
{
    const long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= num_dofs) return;
    if (cmap[d] >= 0)
    {
        if (FILL)
        {
            if (P_ptr[d + 1] - P_ptr[d] != 1) return;
            P_col[P_ptr[d]] = cmap[d];
            P_val[P_ptr[d]] = 1.0;
        }
        else
            row_len[d] = 1;
        return;
    }
    const int n = t.n;
    const long long np = (long long)n * n * n, q = first[d], e = q / np;
    long long v = q % np;
    int idx[3];
    for (int a = 0; a < 3; a++)
    {
        idx[a] = (int)(v % n);
        v /= n;
    }
    int rc[8];
    double rv[8];
    int len = 0;
    for (int corner = 0; corner < 8; corner++)
    {
        double w = 1.0;
        long long cq = 0, stride = 1;
        bool skip = false;
        for (int a = 0; a < 3; a++)
        {
            const int side = (corner >> a) & 1, i = idx[a];
            if (t.lo[i] == t.hi[i])
            {
                if (side) skip = true;
                cq += (long long)t.keep[t.lo[i]] * stride;
            }
            else
            {
                w *= side ? 1.0 - t.wl[i] : t.wl[i];
                cq += (long long)t.keep[side ? t.hi[i] : t.lo[i]] * stride;
            }
            stride *= n;
        }
        if (skip) continue;
        const int fd = point_dof[e * np + cq];
        if (fd < 0) continue; // a Dirichlet corner: an empty lattice row
        const int c = cmap[fd];
        if (c < 0)
        {
            if (not FILL) row_len[d] = -1; // a kept node whose dof is not kept: refused by fdd_amg_setup_row_pointers
            return;
        }
        int k = len++; // insertion in column order, after equal columns (stable)
        for (; k > 0 and rc[k - 1] > c; k--)
        {
            rc[k] = rc[k - 1];
            rv[k] = rv[k - 1];
        }
        rc[k] = c;
        rv[k] = w * 1.0;
    }
    int out = FILL ? P_ptr[d] : 0;
    const int out_end = FILL ? P_ptr[d + 1] : INT_MAX;
    int count = 0;
    for (int k = 0; k < len; k++)
    {
        if (k > 0 and rc[k] == rc[k - 1])
        {
            if (FILL) P_val[out - 1] += rv[k];
            continue;
        }
        if (FILL)
        {
            if (out >= out_end) return;
            P_col[out] = rc[k];
            P_val[out] = rv[k];
        }
        out++;
        count++;
    }
    if (not FILL) row_len[d] = count;
}

// the coarse lattice: kept node cv of element e -> the coarse dof of its fine point (-1: none)
__global__ void lattice_coarse_points_kernel(int *__restrict__ coarse_point_dof, const int *__restrict__ point_dof, const int *__restrict__ cmap, long long num_coarse_points, LatticeTables t)
{
    const long long cq = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (cq >= num_coarse_points) return;
    const int n = t.n, m = t.m;
    const long long npc = (long long)m * m * m, e = cq / npc, cv = cq % npc;
    const long long fq = e * n * n * n + t.keep[cv % m] + (long long)t.keep[(cv / m) % m] * n + (long long)t.keep[cv / (m * m)] * n * n;
    const int fd = point_dof[fq];
    coarse_point_dof[cq] = fd >= 0 ? cmap[fd] : -1;
}

static int lattice_tables(LatticeTables &t, int n, int m, const int *keep, const int *lo, const int *hi, const double *wl)
{
    if (n < 2 || n > kMaxNodes || m < 2 || m > n || !keep || !lo || !hi || !wl) return FDD_ERR_INVALID_ARGUMENT;
    t.n = n;
    t.m = m;
    for (int i = 0; i < kMaxNodes; i++) t.pos[i] = -1;
    for (int a = 0; a < m; a++)
    {
        if (keep[a] < 0 || keep[a] >= n) return FDD_ERR_INVALID_ARGUMENT;
        t.keep[a] = keep[a];
        t.pos[keep[a]] = a;
    }
    for (int i = 0; i < n; i++)
    {
        if (lo[i] < 0 || lo[i] >= m || hi[i] < 0 || hi[i] >= m) return FDD_ERR_INVALID_ARGUMENT;
        t.lo[i] = lo[i];
        t.hi[i] = hi[i];
        t.wl[i] = wl[i];
    }
    return 0;
}

} // namespace

extern "C" {

int fdd_amg_setup_row_pointers(int *ptr, int *ptr_host, const int *row_len, int rows, void *stream)
{
    FDD_REQUIRE(rows >= 0);
    FDD_REQUIRE(ptr != nullptr && ptr_host != nullptr);
    FDD_REQUIRE(rows == 0 || row_len != nullptr);
    std::vector<int> len((size_t)rows);
    if (rows > 0)
    {
        FDD_HIP_CHECK(hipMemcpyAsync(len.data(), row_len, (size_t)rows * sizeof(int), hipMemcpyDeviceToHost, fdd_stream(stream)));
        FDD_HIP_CHECK(hipStreamSynchronize(fdd_stream(stream)));
    }
    long long total = 0;
    ptr_host[0] = 0;
    for (int i = 0; i < rows; i++)
    {
        total += len[(size_t)i];
        if (len[(size_t)i] < 0 || total > INT_MAX)
        {
            fdd_set_error("invalid argument: the entry count of the sparse result exceeds the int range of its row pointers (row %d)", i);
            return FDD_ERR_INVALID_ARGUMENT;
        }
        ptr_host[i + 1] = (int)total;
    }
    FDD_HIP_CHECK(hipMemcpyAsync(ptr, ptr_host, ((size_t)rows + 1) * sizeof(int), hipMemcpyHostToDevice, fdd_stream(stream)));
    FDD_HIP_CHECK(hipStreamSynchronize(fdd_stream(stream)));
    return 0;
}

int fdd_amg_setup_spgemm_count(int *row_len, int *cursor_ws, const int *A_ptr, const int *A_col, const int *B_ptr, const int *B_col, int a_rows, int b_rows, void *stream)
{
    FDD_REQUIRE(a_rows >= 0 && b_rows >= 0);
    if (a_rows == 0) return 0;
    FDD_REQUIRE(row_len != nullptr && cursor_ws != nullptr && A_ptr != nullptr && B_ptr != nullptr);
    spgemm_kernel<false><<<blocks_for(a_rows), kBlock, 0, fdd_stream(stream)>>>(row_len, nullptr, nullptr, cursor_ws, nullptr, A_ptr, A_col, nullptr, B_ptr, B_col, nullptr, a_rows, b_rows);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_amg_setup_spgemm_fill(int *C_col, double *C_val, int *cursor_ws, const int *C_ptr, const int *A_ptr, const int *A_col, const double *A_val, const int *B_ptr, const int *B_col, const double *B_val, int a_rows, int b_rows,
                              void *stream)
{
    FDD_REQUIRE(a_rows >= 0 && b_rows >= 0);
    if (a_rows == 0) return 0;
    FDD_REQUIRE(C_ptr != nullptr && cursor_ws != nullptr && A_ptr != nullptr && B_ptr != nullptr); // col / val: NULL only for a matrix without entries
    spgemm_kernel<true><<<blocks_for(a_rows), kBlock, 0, fdd_stream(stream)>>>(nullptr, C_col, C_val, cursor_ws, C_ptr, A_ptr, A_col, A_val, B_ptr, B_col, B_val, a_rows, b_rows);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_amg_setup_transpose_count(int *row_len, const int *A_ptr, const int *A_col, const double *A_val, int a_rows, int a_cols, double drop_tol, void *stream)
{
    FDD_REQUIRE(a_rows >= 0 && a_cols >= 0);
    if (a_cols == 0) return 0;
    FDD_REQUIRE(row_len != nullptr);
    FDD_HIP_CHECK(hipMemsetAsync(row_len, 0, (size_t)a_cols * sizeof(int), fdd_stream(stream)));
    if (a_rows == 0) return 0;
    FDD_REQUIRE(A_ptr != nullptr); // A_col: NULL only for a matrix without entries
    transpose_count_kernel<<<blocks_for(a_rows), kBlock, 0, fdd_stream(stream)>>>(row_len, A_ptr, A_col, A_val, a_rows, a_cols, drop_tol);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_amg_setup_transpose_fill(int *T_col, double *T_val, int *cursor_ws, int *src_ws, const int *T_ptr, const int *A_ptr, const int *A_col, const double *A_val, int a_rows, int a_cols, int nnz_t, double drop_tol,
                                 void *stream)
{
    FDD_REQUIRE(a_rows >= 0 && a_cols >= 0 && nnz_t >= 0);
    if (a_rows == 0 || a_cols == 0 || nnz_t == 0) return 0;
    FDD_REQUIRE(T_col != nullptr && cursor_ws != nullptr && src_ws != nullptr && T_ptr != nullptr && A_ptr != nullptr && A_col != nullptr);
    FDD_REQUIRE(T_val == nullptr || A_val != nullptr);
    FDD_HIP_CHECK(hipMemcpyAsync(cursor_ws, T_ptr, (size_t)a_cols * sizeof(int), hipMemcpyDeviceToDevice, fdd_stream(stream)));
    transpose_place_kernel<<<blocks_for(a_rows), kBlock, 0, fdd_stream(stream)>>>(src_ws, cursor_ws, A_ptr, A_col, A_val, a_rows, a_cols, drop_tol, nnz_t);
    FDD_LAUNCH_CHECK();
    transpose_order_kernel<<<blocks_for(a_cols), kBlock, 0, fdd_stream(stream)>>>(T_col, T_val, src_ws, T_ptr, A_ptr, A_val, a_rows, a_cols);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_amg_setup_fem_stencils(double *K, unsigned int *mask, const double *x, const double *y, const double *z, const int *point_dof, int poly_degree, int num_elements, double epsilon, void *stream)
{
    FDD_REQUIRE(poly_degree >= 1 && poly_degree <= 32 && num_elements >= 0);
    if (num_elements == 0) return 0;
    FDD_REQUIRE(K != nullptr && mask != nullptr && x != nullptr && y != nullptr && z != nullptr && point_dof != nullptr);
    const long long n = poly_degree + 1, points = (long long)num_elements * n * n * n;
    fem_stencil_kernel<<<blocks_for(points), kBlock, 0, fdd_stream(stream)>>>(K, mask, x, y, z, point_dof, poly_degree, points, epsilon);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_amg_setup_fem_count(int *row_len, const int *dof_ptr, const int *dof_points, const unsigned int *mask, const int *point_dof, int poly_degree, int num_dofs, void *stream)
{
    FDD_REQUIRE(poly_degree >= 1 && poly_degree <= 32 && num_dofs >= 0);
    if (num_dofs == 0) return 0;
    FDD_REQUIRE(row_len != nullptr && dof_ptr != nullptr && dof_points != nullptr && mask != nullptr && point_dof != nullptr);
    fem_row_kernel<false><<<blocks_for(num_dofs), kBlock, 0, fdd_stream(stream)>>>(row_len, nullptr, nullptr, nullptr, dof_ptr, dof_points, mask, nullptr, point_dof, poly_degree, num_dofs);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_amg_setup_fem_fill(int *A_col, double *A_val, const int *A_ptr, const int *dof_ptr, const int *dof_points, const unsigned int *mask, const double *K, const int *point_dof, int poly_degree, int num_dofs, void *stream)
{
    FDD_REQUIRE(poly_degree >= 1 && poly_degree <= 32 && num_dofs >= 0);
    if (num_dofs == 0) return 0;
    FDD_REQUIRE(A_col != nullptr && A_val != nullptr && A_ptr != nullptr && dof_ptr != nullptr && dof_points != nullptr && mask != nullptr && K != nullptr && point_dof != nullptr);
    fem_row_kernel<true><<<blocks_for(num_dofs), kBlock, 0, fdd_stream(stream)>>>(nullptr, A_col, A_val, A_ptr, dof_ptr, dof_points, mask, K, point_dof, poly_degree, num_dofs);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_amg_setup_inv_sqrt_diagonal(double *D, const int *A_ptr, const int *A_col, const double *A_val, int rows, void *stream)
{
    FDD_REQUIRE(rows >= 0);
    if (rows == 0) return 0;
    FDD_REQUIRE(D != nullptr && A_ptr != nullptr && A_col != nullptr && A_val != nullptr);
    inv_sqrt_diagonal_kernel<<<blocks_for(rows), kBlock, 0, fdd_stream(stream)>>>(D, A_ptr, A_col, A_val, rows);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_amg_setup_unit_values(int *flag, const double *val, long long nnz, void *stream)
{
    FDD_REQUIRE(flag != nullptr && nnz >= 0);
    FDD_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(flag), 1, 1, fdd_stream(stream)));
    if (nnz == 0) return 0;
    FDD_REQUIRE(val != nullptr);
    unit_values_kernel<<<fdd_stream_grid(nnz, kBlock), kBlock, 0, fdd_stream(stream)>>>(flag, val, nnz);
    FDD_LAUNCH_CHECK();
    return 0;
}

#define FDD_LATTICE_TABLES(t)                                                                                  \
    LatticeTables t;                                                                                           \
    if (lattice_tables(t, n, m, keep, lo, hi, wl) != 0)                                                        \
    {                                                                                                          \
        fdd_set_error("invalid argument: lattice tables (n = %d, m = %d, at most %d nodes)", n, m, kMaxNodes); \
        return FDD_ERR_INVALID_ARGUMENT;                                                                       \
    }

int fdd_amg_setup_lattice_dofs(int *first, int *kept, const int *point_dof, long long num_elements, int num_dofs, int n, int m, const int *keep, const int *lo, const int *hi, const double *wl, void *stream)
{
    FDD_REQUIRE(num_elements >= 0 && num_dofs >= 0);
    FDD_LATTICE_TABLES(t);
    if (num_dofs == 0) return 0;
    FDD_REQUIRE(first != nullptr && kept != nullptr && point_dof != nullptr);
    FDD_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(first), INT_MAX, (size_t)num_dofs, fdd_stream(stream)));
    FDD_HIP_CHECK(hipMemsetAsync(kept, 0, (size_t)num_dofs * sizeof(int), fdd_stream(stream)));
    const long long points = num_elements * n * n * n;
    FDD_REQUIRE(points <= INT_MAX);
    if (points == 0) return 0;
    lattice_first_kernel<<<blocks_for(points), kBlock, 0, fdd_stream(stream)>>>(first, kept, point_dof, points, num_dofs, t);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_amg_setup_lattice_coarse_flags(int *flag, const int *first, const int *kept, int num_dofs, void *stream)
{
    FDD_REQUIRE(num_dofs >= 0);
    if (num_dofs == 0) return 0;
    FDD_REQUIRE(flag != nullptr && first != nullptr && kept != nullptr);
    lattice_coarse_flag_kernel<<<blocks_for(num_dofs), kBlock, 0, fdd_stream(stream)>>>(flag, first, kept, num_dofs);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_amg_setup_lattice_cmap(int *cmap, int *owner_dof, int *unplaced, const int *cstart, const int *first, const int *kept, long long num_points, int num_dofs, void *stream)
{
    FDD_REQUIRE(num_dofs >= 0 && num_points >= 0);
    FDD_REQUIRE(owner_dof != nullptr && unplaced != nullptr);
    FDD_HIP_CHECK(hipMemsetAsync(unplaced, 0, sizeof(int), fdd_stream(stream)));
    if (num_points > 0) FDD_HIP_CHECK(hipMemsetAsync(owner_dof, 0xFF, (size_t)num_points * sizeof(int), fdd_stream(stream))); // -1
    if (num_dofs == 0) return 0;
    FDD_REQUIRE(cmap != nullptr && cstart != nullptr && first != nullptr && kept != nullptr);
    lattice_cmap_kernel<<<blocks_for(num_dofs), kBlock, 0, fdd_stream(stream)>>>(cmap, owner_dof, unplaced, cstart, first, kept, num_dofs);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_amg_setup_lattice_interp_count(int *row_len, const int *cmap, const int *first, const int *point_dof, int num_dofs, int n, int m, const int *keep, const int *lo, const int *hi, const double *wl, void *stream)
{
    FDD_REQUIRE(num_dofs >= 0);
    FDD_LATTICE_TABLES(t);
    if (num_dofs == 0) return 0;
    FDD_REQUIRE(row_len != nullptr && cmap != nullptr && first != nullptr && point_dof != nullptr);
    lattice_interp_kernel<false><<<blocks_for(num_dofs), kBlock, 0, fdd_stream(stream)>>>(row_len, nullptr, nullptr, nullptr, cmap, first, point_dof, num_dofs, t);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_amg_setup_lattice_interp_fill(int *P_col, double *P_val, const int *P_ptr, const int *cmap, const int *first, const int *point_dof, int num_dofs, int n, int m, const int *keep, const int *lo, const int *hi, const double *wl, void *stream)
{
    FDD_REQUIRE(num_dofs >= 0);
    FDD_LATTICE_TABLES(t);
    if (num_dofs == 0) return 0;
    FDD_REQUIRE(P_col != nullptr && P_val != nullptr && P_ptr != nullptr && cmap != nullptr && first != nullptr && point_dof != nullptr);
    lattice_interp_kernel<true><<<blocks_for(num_dofs), kBlock, 0, fdd_stream(stream)>>>(nullptr, P_col, P_val, P_ptr, cmap, first, point_dof, num_dofs, t);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_amg_setup_lattice_coarse_points(int *coarse_point_dof, const int *point_dof, const int *cmap, long long num_elements, int n, int m, const int *keep, const int *lo, const int *hi, const double *wl, void *stream)
{
    FDD_REQUIRE(num_elements >= 0);
    FDD_LATTICE_TABLES(t);
    const long long points = num_elements * m * m * m;
    if (points == 0) return 0;
    FDD_REQUIRE(coarse_point_dof != nullptr && point_dof != nullptr && cmap != nullptr);
    lattice_coarse_points_kernel<<<blocks_for(points), kBlock, 0, fdd_stream(stream)>>>(coarse_point_dof, point_dof, cmap, points, t);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_amg_setup_memory_info(size_t *free_bytes, size_t *total_bytes)
{
    FDD_REQUIRE(free_bytes != nullptr && total_bytes != nullptr);
    FDD_HIP_CHECK(hipMemGetInfo(free_bytes, total_bytes));
    return 0;
}

} // extern "C"
