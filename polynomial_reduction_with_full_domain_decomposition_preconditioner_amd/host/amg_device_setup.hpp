/*
 * amg_device_setup.hpp -- the sparse steps of the low-order AMG setup in HBM (fdd_amg_setup_* of include/fdd_hip.h,
 * csrc/fdd_amg_setup.hip), each the device form of a routine of low_order.hpp with the same result bit for bit:
 *
 *   assemble_fem   low_order::assemble_fem (element stencils, then the rows of the dofs as from_triplets merges them)
 *   multiply       low_order::multiply (Gustavson)
 *   transpose      low_order::transpose
 *   inv_sqrt_diag  D = 1 / sqrt(diag(A)) of low_order::build
 *   geometric_level  low_order::geometric_level on a conforming lattice (interpolator, coarse lattice, Transfer maps)
 *
 * Used by Subdomain::amg_build under the switch "amg_device_setup" ("AMG setup on the device").
 */
#ifndef FDD_AMG_DEVICE_SETUP_HPP
#define FDD_AMG_DEVICE_SETUP_HPP

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "fdd_device.hpp"
#include "low_order.hpp"

namespace fdd
{
namespace amg_setup
{

// CSR in HBM with the host's copy of the row pointers (the SpMV plans and the next step's sizes are made from it)
struct DeviceCSR
{
    int rows = 0, cols = 0;
    std::vector<int> ptr_hst;
    memory ptr, col, val;
    long long nnz() const { return ptr_hst.empty() ? 0 : ptr_hst.back(); }
    void free() { *this = DeviceCSR(); } // before the end of a scope: bounds the peak of a build
};

// the least free device memory seen at the sample points of a build (FDD_SETUP_TIMING: its peak)
inline size_t &least_free()
{
    static thread_local size_t f = (size_t)-1;
    return f;
}
inline void note_memory()
{
    static const bool timing = getenv("FDD_SETUP_TIMING") != nullptr;
    if (not timing) return;
    FDD_CALL(fdd_stream_sync(dev().stream));
    size_t free_b = 0, total_b = 0;
    FDD_CALL(fdd_amg_setup_memory_info(&free_b, &total_b));
    least_free() = std::min(least_free(), free_b);
}

inline DeviceCSR upload(const low_order::HostCSR &H, bool values = true)
{
    DeviceCSR D;
    D.rows = H.rows;
    D.cols = H.cols;
    D.ptr_hst = H.ptr;
    const size_t nnz = (size_t)H.nnz();
    D.ptr = dev().malloc<int>((size_t)H.rows + 1);
    D.ptr.copyFrom(H.ptr.data(), ((size_t)H.rows + 1) * sizeof(int));
    D.col = dev().malloc<int>(std::max<size_t>(nnz, 1));
    if (nnz) D.col.copyFrom(H.col.data(), nnz * sizeof(int));
    if (values)
    {
        D.val = dev().malloc<double>(std::max<size_t>(nnz, 1));
        if (nnz) D.val.copyFrom(H.val.data(), nnz * sizeof(double));
    }
    return D;
}

inline low_order::HostCSR download(const DeviceCSR &D)
{
    low_order::HostCSR H;
    H.rows = D.rows;
    H.cols = D.cols;
    H.ptr = D.ptr_hst;
    const size_t nnz = (size_t)D.nnz();
    H.col.resize(nnz);
    H.val.resize(nnz);
    if (nnz)
    {
        D.col.copyTo(H.col.data(), nnz * sizeof(int));
        D.val.copyTo(H.val.data(), nnz * sizeof(double));
    }
    return H;
}

// row lengths (device) -> ptr on both sides; the entry count is checked against the int range there
inline void row_pointers(DeviceCSR &C, memory &row_len)
{
    C.ptr_hst.resize((size_t)C.rows + 1);
    C.ptr = dev().malloc<int>((size_t)C.rows + 1);
    FDD_CALL(fdd_amg_setup_row_pointers(C.ptr.as<int>(), C.ptr_hst.data(), row_len.as<int>(), C.rows, dev().stream));
    row_len.free();
    const size_t nnz = (size_t)C.nnz();
    C.col = dev().malloc<int>(std::max<size_t>(nnz, 1));
    C.val = dev().malloc<double>(std::max<size_t>(nnz, 1));
    note_memory();
}

// C = A B
inline DeviceCSR multiply(const DeviceCSR &A, const DeviceCSR &B)
{
    DeviceCSR C;
    C.rows = A.rows;
    C.cols = B.cols;
    memory len = dev().malloc<int>(std::max(A.rows, 1)), cursor = dev().malloc<int>(std::max<size_t>((size_t)A.nnz(), 1));
    FDD_CALL(fdd_amg_setup_spgemm_count(len.as<int>(), cursor.as<int>(), A.ptr.as<int>(), A.col.as<int>(), B.ptr.as<int>(), B.col.as<int>(), A.rows, B.rows, dev().stream));
    row_pointers(C, len);
    FDD_CALL(fdd_amg_setup_spgemm_fill(C.col.as<int>(), C.val.as<double>(), cursor.as<int>(), C.ptr.as<int>(), A.ptr.as<int>(), A.col.as<int>(), A.val.as<double>(), B.ptr.as<int>(), B.col.as<int>(), B.val.as<double>(), A.rows,
                                       B.rows, dev().stream));
    return C;
}

// T = A^T (values moved when A has them); drop_tol >= 0: only the entries with |a| > drop_tol (CSR_Matrix::transpose)
inline DeviceCSR transpose(const DeviceCSR &A, double drop_tol = -1.0)
{
    DeviceCSR T;
    T.rows = A.cols;
    T.cols = A.rows;
    const double *val = A.val.isInitialized() ? A.val.as<double>() : nullptr;
    memory len = dev().malloc<int>(std::max(A.cols, 1));
    FDD_CALL(fdd_amg_setup_transpose_count(len.as<int>(), A.ptr.as<int>(), A.col.as<int>(), val, A.rows, A.cols, drop_tol, dev().stream));
    row_pointers(T, len);
    if (val == nullptr) T.val.free();
    memory cursor = dev().malloc<int>(std::max(A.cols, 1)), src = dev().malloc<int>(std::max<size_t>((size_t)T.nnz(), 1));
    FDD_CALL(fdd_amg_setup_transpose_fill(T.col.as<int>(), val ? T.val.as<double>() : nullptr, cursor.as<int>(), src.as<int>(), T.ptr.as<int>(), A.ptr.as<int>(), A.col.as<int>(), val, A.rows, A.cols, (int)T.nnz(), drop_tol,
                                          dev().stream));
    return T;
}

// the level-0 FEM matrix of low_order::assemble_fem from the level-0 points (host arrays, uploaded here) and their dofs
// (pdof, in HBM); `points`: the point -> dof map in CSR form (the lattice rows of Subdomain::amg_build)
inline DeviceCSR assemble_fem(const double *x, const double *y, const double *z, const memory &pdof, const low_order::HostCSR &points, int num_dofs, int poly_degree, int num_elements, double epsilon)
{
    const int n = poly_degree + 1;
    const size_t np = (size_t)num_elements * n * n * n;
    memory dx = dev().malloc<double>(np), dy = dev().malloc<double>(np), dz = dev().malloc<double>(np);
    dx.copyFrom(x, np * sizeof(double));
    dy.copyFrom(y, np * sizeof(double));
    dz.copyFrom(z, np * sizeof(double));
    memory K = dev().malloc<double>(np * 27), mask = dev().malloc<unsigned int>(np);
    note_memory();
    FDD_CALL(fdd_amg_setup_fem_stencils(K.as<double>(), mask.as<unsigned int>(), dx.as<double>(), dy.as<double>(), dz.as<double>(), pdof.as<int>(), poly_degree, num_elements, epsilon, dev().stream));
    dx = dy = dz = memory(); // bounds the peak
    // dof -> its points in ascending order: the transpose of the point -> dof map
    DeviceCSR P = upload(points, false);
    DeviceCSR Pt = transpose(P);
    P.free();
    DeviceCSR A;
    A.rows = A.cols = num_dofs;
    memory len = dev().malloc<int>(std::max(num_dofs, 1));
    FDD_CALL(fdd_amg_setup_fem_count(len.as<int>(), Pt.ptr.as<int>(), Pt.col.as<int>(), mask.as<unsigned int>(), pdof.as<int>(), poly_degree, num_dofs, dev().stream));
    row_pointers(A, len);
    note_memory();
    FDD_CALL(fdd_amg_setup_fem_fill(A.col.as<int>(), A.val.as<double>(), A.ptr.as<int>(), Pt.ptr.as<int>(), Pt.col.as<int>(), mask.as<unsigned int>(), K.as<double>(), pdof.as<int>(), poly_degree, num_dofs, dev().stream));
    return A;
}

// A conforming lattice in HBM: its point -> dof array (num_elements * n^3 points, -1: no dof) over `cols` dofs
struct DeviceLattice
{
    int n = 0, cols = 0;
    std::vector<double> ref;
    long long num_elements = 0;
    memory point_dof;
    // the host's description of it for low_order::plan_level (no rows), or the whole of it (rows downloaded)
    low_order::Lattice host(bool with_rows) const
    {
        low_order::Lattice L;
        L.dim = 3;
        L.n = n;
        L.ref = ref;
        L.num_elements = num_elements;
        L.rows.rows = (int)(num_elements * n * n * n);
        L.rows.cols = cols;
        if (with_rows)
        {
            const size_t np = (size_t)L.rows.rows;
            std::vector<int> pd(np);
            if (np) point_dof.copyTo(pd.data(), np * sizeof(int));
            L.rows.ptr.assign(np + 1, 0);
            for (size_t q = 0; q < np; q++) L.rows.ptr[q + 1] = L.rows.ptr[q] + (pd[q] >= 0 ? 1 : 0);
            L.rows.col.resize((size_t)L.rows.ptr[np]);
            for (size_t q = 0; q < np; q++)
                if (pd[q] >= 0) L.rows.col[(size_t)L.rows.ptr[q]] = pd[q];
            L.rows.val.assign(L.rows.col.size(), 1.0);
        }
        return L;
    }
};

// low_order::geometric_level on a conforming 3-D lattice: P (dofs x coarse dofs), the coarse lattice, and the Transfer maps
// (fetched into `transfer`, which Hierarchy::set_lattice_transfer takes)
inline DeviceCSR geometric_level(const DeviceLattice &fine, int num_dofs, DeviceLattice &coarse, low_order::Transfer &transfer)
{
    const int n = fine.n;
    const std::vector<int> keep = low_order::coarse_nodes(n, fine.ref);
    const int m = (int)keep.size();
    std::vector<int> lo(n), hi(n), pos(n, -1);
    std::vector<double> wl(n);
    for (int a = 0; a < m; a++) pos[keep[a]] = a;
    for (int i = 0, a = 0; i < n; i++) // the host routine's 1-D tables, verbatim
    {
        if (pos[i] >= 0)
        {
            lo[i] = hi[i] = pos[i];
            wl[i] = 1.0;
            a = pos[i];
            continue;
        }
        lo[i] = a;
        hi[i] = a + 1;
        wl[i] = (fine.ref[keep[a + 1]] - fine.ref[i]) / (fine.ref[keep[a + 1]] - fine.ref[keep[a]]);
    }
    const long long total = fine.num_elements * n * n * n, kept_points = fine.num_elements * m * m * m;
    void *s = dev().stream;
    memory first = dev().malloc<int>(std::max(num_dofs, 1)), kept = dev().malloc<int>(std::max(num_dofs, 1));
    FDD_CALL(fdd_amg_setup_lattice_dofs(first.as<int>(), kept.as<int>(), fine.point_dof.as<int>(), fine.num_elements, num_dofs, n, m, keep.data(), lo.data(), hi.data(), wl.data(), s));
    memory flag = dev().malloc<int>(std::max(num_dofs, 1));
    FDD_CALL(fdd_amg_setup_lattice_coarse_flags(flag.as<int>(), first.as<int>(), kept.as<int>(), num_dofs, s));
    DeviceCSR start; // exclusive prefix counts of the flags: the coarse numbering
    start.rows = num_dofs;
    start.ptr_hst.resize((size_t)num_dofs + 1);
    start.ptr = dev().malloc<int>((size_t)num_dofs + 1);
    FDD_CALL(fdd_amg_setup_row_pointers(start.ptr.as<int>(), start.ptr_hst.data(), flag.as<int>(), num_dofs, s));
    flag.free();
    const int nc = start.ptr_hst.back();
    memory cmap = dev().malloc<int>(std::max(num_dofs, 1)), owner = dev().malloc<int>(std::max<size_t>((size_t)total, 1)), unplaced = dev().malloc<int>(1);
    FDD_CALL(fdd_amg_setup_lattice_cmap(cmap.as<int>(), owner.as<int>(), unplaced.as<int>(), start.ptr.as<int>(), first.as<int>(), kept.as<int>(), total, num_dofs, s));
    start.free();
    DeviceCSR P;
    P.rows = num_dofs;
    P.cols = nc;
    memory len = dev().malloc<int>(std::max(num_dofs, 1));
    FDD_CALL(fdd_amg_setup_lattice_interp_count(len.as<int>(), cmap.as<int>(), first.as<int>(), fine.point_dof.as<int>(), num_dofs, n, m, keep.data(), lo.data(), hi.data(), wl.data(), s));
    row_pointers(P, len);
    FDD_CALL(fdd_amg_setup_lattice_interp_fill(P.col.as<int>(), P.val.as<double>(), P.ptr.as<int>(), cmap.as<int>(), first.as<int>(), fine.point_dof.as<int>(), num_dofs, n, m, keep.data(), lo.data(), hi.data(), wl.data(), s));
    coarse = DeviceLattice();
    coarse.n = m;
    coarse.cols = nc;
    coarse.num_elements = fine.num_elements;
    coarse.ref.resize(m);
    for (int a = 0; a < m; a++) coarse.ref[a] = fine.ref[keep[a]];
    coarse.point_dof = dev().malloc<int>(std::max<size_t>((size_t)kept_points, 1));
    FDD_CALL(fdd_amg_setup_lattice_coarse_points(coarse.point_dof.as<int>(), fine.point_dof.as<int>(), cmap.as<int>(), fine.num_elements, n, m, keep.data(), lo.data(), hi.data(), wl.data(), s));
    note_memory();
    // the matrix-free form (low_order::Transfer): on this lattice every row is a unit entry or empty, so it is plain
    // wherever every dof sits on a lattice point
    int unplaced_h = 0;
    unplaced.copyTo(&unplaced_h, sizeof(int));
    transfer = low_order::Transfer();
    if (unplaced_h == 0 and total < (1LL << 31))
    {
        transfer.n = n;
        transfer.m = m;
        transfer.lo = lo;
        transfer.hi = hi;
        transfer.wl = wl;
        transfer.num_elements = fine.num_elements;
        transfer.owner_dof.resize((size_t)total);
        owner.copyTo(transfer.owner_dof.data(), (size_t)total * sizeof(int));
        transfer.coarse_dof.resize((size_t)kept_points);
        coarse.point_dof.copyTo(transfer.coarse_dof.data(), (size_t)kept_points * sizeof(int));
    }
    return P;
}

inline memory inv_sqrt_diag(const DeviceCSR &A)
{
    memory D = dev().malloc<double>(std::max(A.rows, 1));
    FDD_CALL(fdd_amg_setup_inv_sqrt_diagonal(D.as<double>(), A.ptr.as<int>(), A.col.as<int>(), A.val.as<double>(), A.rows, dev().stream));
    return D;
}

} // namespace amg_setup
} // namespace fdd

#endif
