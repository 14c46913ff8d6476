"""Times the field kernels (fdd_field_mass, _gradient, _weak_divergence, _convect, _weak_convect; csrc/fdd_field.hip) and, in
the same process for comparison, the six-array fused stiffness kernel (fdd_dom_stiffness_matrix, 64 B per point) with HIP events:

    python tools/field_ops_time.py [--elements 32] [--degrees 7 15] [--launches 20] [--windows 7]

Per degree and mesh (the unit box, and the box under the Kershaw map with eps = 0.3, built on the GPU) every kernel is
warmed up, then timed in `windows` windows of `launches` back-to-back launches between two events, the kernels taking
turns window by window so that a drift of the machine falls on all of them alike.  Printed: the median, fastest and slowest
window per launch, the algorithmic bytes per point and the rate they make, and the gradient's time over the stiffness
kernel's.  One JSON line per degree and mesh at the end.  The stiffness kernel's time does not depend on the values of its
factor arrays; they are filled with positive numbers, not with the mesh's factors.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BYTES_PER_POINT = {"mass": 32, "gradient": 56, "weak_divergence": 56, "convect": 64, "weak_convect": 64, "stiffness": 64}


def gll(N):
    """Gauss-Lobatto-Legendre nodes, weights and the differentiation matrix D[i, p] = l_p'(z_i), row-major"""
    P = np.polynomial.legendre.Legendre.basis(N)
    z = np.concatenate([[-1.0], np.sort(P.deriv().roots().real), [1.0]])
    w = 2.0 / (N * (N + 1) * P(z) ** 2)
    D = np.zeros((N + 1, N + 1))
    for i in range(N + 1):
        for p in range(N + 1):
            if i != p:
                D[i, p] = P(z[i]) / (P(z[p]) * (z[i] - z[p]))
    D[0, 0], D[N, N] = -0.25 * N * (N + 1), 0.25 * N * (N + 1)
    return z, w, D.reshape(-1)


def gauss_tables(N, z_gll, D):
    """weak_convect's rule: M = (3n+1)/2 Gauss-Legendre weights, P[q, i] = l_i(zeta_q) (barycentric) and P' = P D"""
    n = N + 1
    zeta, omega = np.polynomial.legendre.leggauss((3 * n + 1) // 2)
    lam = np.array([1.0 / np.prod([z_gll[i] - z_gll[j] for j in range(n) if j != i]) for i in range(n)])
    diff = zeta[:, None] - z_gll[None, :]
    hit = np.abs(diff) < 1e-14  # the centre of an odd rule on an odd grid
    P = lam[None, :] / np.where(hit, 1.0, diff)
    P = P / P.sum(axis=1)[:, None]
    P[hit.any(axis=1)] = hit[hit.any(axis=1)].astype(float)
    return omega, P, P @ D.reshape(n, n)


def kershaw(torch, eps, x, y, z):
    """the generalized Kershaw map of the unit cube (host/box_mesh.hpp), on tensors"""
    right = lambda s: torch.where(s <= 0.5, (2.0 - eps) * s, 1.0 + eps * (s - 1.0))
    left = lambda s: 1.0 - right(1.0 - s)
    layer = torch.clamp(torch.floor(x * 6.0), 0, 5)
    lam = (x - layer / 6.0) * 6.0
    step = lambda a, b, t: a + (b - a) * torch.clamp(t, 0.0, 1.0)

    def section(s):
        L, R = left(s), right(s)
        out = R.clone()
        for which, value in ((layer == 0, L), ((layer == 1) | (layer == 4), step(L, R, lam)), (layer == 2, step(R, L, 0.5 * lam)), (layer == 3, step(R, L, 0.5 * (1.0 + lam)))):
            out = torch.where(which, value, out)
        return out

    return x, section(y), section(z)


def coordinates(torch, gpu, E, N, z_gll):
    """x, y, z of the E^3-element unit box at degree N: element-major, x fastest inside an element"""
    n = N + 1
    xi = torch.tensor(0.5 * (z_gll + 1.0), device=gpu)
    e = torch.arange(E, device=gpu, dtype=torch.float64)
    line = ((e[:, None] + xi[None, :]) / E)  # [element, node] along one direction
    shape = (E, E, E, n, n, n)  # [ez, ey, ex, k, j, i]
    x = line[None, None, :, None, None, :].expand(shape).reshape(-1)
    y = line[None, :, None, None, :, None].expand(shape).reshape(-1)
    z = line[:, None, None, :, None, None].expand(shape).reshape(-1)
    return x.contiguous(), y.contiguous(), z.contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--elements", type=int, default=32, help="elements per direction")
    ap.add_argument("--degrees", type=int, nargs="+", default=[7, 15])
    ap.add_argument("--launches", type=int, default=20, help="launches per timed window")
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("field_ops_time.py needs a GPU")
    from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd.kernels import k

    gpu = torch.device("cuda:0")
    records = []
    for N in args.degrees:
        zg, wg, Dh = gll(N)
        E3, n3 = args.elements**3, (N + 1) ** 3
        npts = E3 * n3
        D, w = torch.tensor(Dh, device=gpu), torch.tensor(wg, device=gpu)
        omega, P, Pd = (torch.tensor(np.ascontiguousarray(t), device=gpu) for t in gauss_tables(N, zg, Dh))
        gen = torch.Generator(device=gpu).manual_seed(1234 + N)
        rand = lambda lo, hi: torch.rand(npts, device=gpu, dtype=torch.float64, generator=gen) * (hi - lo) + lo
        u, v = rand(-1.0, 1.0), [rand(-1.0, 1.0) for _ in range(3)]
        G = [rand(0.5, 1.5) for _ in range(3)] + [rand(-0.1, 0.1) for _ in range(3)]
        out = [torch.zeros(npts, device=gpu, dtype=torch.float64) for _ in range(3)]
        box = coordinates(torch, gpu, args.elements, N, zg)
        for mesh, xyz in (("box", list(box)), ("kershaw", [c.contiguous() for c in kershaw(torch, 0.3, *box)])):
            launch = {
                "mass": lambda: k("fdd_field_mass", out[0], xyz, D, w, E3, N),
                "gradient": lambda: k("fdd_field_gradient", out, u, xyz, D, E3, N),
                "weak_divergence": lambda: k("fdd_field_weak_divergence", out[0], v, xyz, D, w, E3, N),
                "convect": lambda: k("fdd_field_convect", out[0], v, u, xyz, D, E3, N),
                "weak_convect": lambda: k("fdd_field_weak_convect", out[0], v, u, xyz, D, P, Pd, omega, len(omega), E3, N),
                "stiffness": lambda: k("fdd_dom_stiffness_matrix", out[0], u, D, G, E3, N),
            }
            for fn in launch.values():  # warm-up: code objects loaded, every array touched
                for _ in range(3):
                    fn()
            launch["mass"]()
            least_mass = float(out[0].min())  # > 0: the mesh's Jacobian is positive at every point
            us = {name: [] for name in launch}
            for _ in range(args.windows):
                for name, fn in launch.items():
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(args.launches):
                        fn()
                    t1.record()
                    t1.synchronize()
                    us[name].append(1e3 * t0.elapsed_time(t1) / args.launches)
            rec = {"elements": args.elements, "degree": N, "mesh": mesh, "points": npts, "min_mass": least_mass, "launches": args.launches, "windows": args.windows, "kernels": {}}
            print("%d^3 elements, degree %d, %s: %d points, min(mass) = %.3e" % (args.elements, N, mesh, npts, least_mass))
            for name, t in us.items():
                med = float(np.median(t))
                rec["kernels"][name] = {"us_median": med, "us_min": min(t), "us_max": max(t), "bytes_per_point": BYTES_PER_POINT[name], "TB_per_s": BYTES_PER_POINT[name] * npts / med * 1e-6}
                print("  %-16s %9.1f us  (%.1f .. %.1f)  %2d B/point  %5.2f TB/s" % (name, med, min(t), max(t), BYTES_PER_POINT[name], rec["kernels"][name]["TB_per_s"]))
            rec["gradient_over_stiffness"] = rec["kernels"]["gradient"]["us_median"] / rec["kernels"]["stiffness"]["us_median"]
            rec["weak_convect_over_gradient"] = rec["kernels"]["weak_convect"]["us_median"] / rec["kernels"]["gradient"]["us_median"]
            print("  gradient / stiffness = %.2f, weak_convect / gradient = %.2f" % (rec["gradient_over_stiffness"], rec["weak_convect_over_gradient"]))
            records.append(rec)
        del u, v, G, out, box, xyz
        torch.cuda.empty_cache()
    for rec in records:
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
