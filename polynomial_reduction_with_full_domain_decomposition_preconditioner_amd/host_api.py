"""Python plumbing over libfdd_host.so (include/fdd_host.h): numpy vectors in
and out, communicator set-up from torch.distributed.  The solver itself is the
C++ host layer on the HIP kernels; nothing here computes."""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

import numpy as np

from . import lib

vp = ctypes.c_void_p

INFO_NAMES = [
    "num_local_points",
    "num_local_nodes",
    "num_bdary_nodes",
    "num_interface_slots",
    "num_total_nodes",
    "num_total_elements",
    "num_local_elements",
    "num_levels",
    "sub_num_values",
    "sub_num_dofs",
    "num_iterations",
    "dim",
]

_ALLREDUCE = ctypes.CFUNCTYPE(ctypes.c_int, vp, vp, ctypes.c_longlong)
_ALLGATHER = ctypes.CFUNCTYPE(ctypes.c_int, vp, vp, vp, ctypes.c_longlong)
_BARRIER = ctypes.CFUNCTYPE(ctypes.c_int, vp)
_EXCHANGE = ctypes.CFUNCTYPE(ctypes.c_int, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_longlong))

SUB_INFO_NAMES = [
    "is_composite",
    "num_elems",
    "num_ext_elems",
    "num_points",
    "sub_dofs",
    "sub_ext_dofs",
    "interface_dofs",
    "sup_dofs",
    "sup_ext_dofs",
    "unique_dofs",
    "coarse_dofs",
    "num_values",
    "own_points",
    "num_peers",
]

WITH_SUBDOMAIN, BLOCK_LOCAL, FORCE_COMPOSITE = 1, 2, 4

_keepalive = []


def _H():
    return lib.host()


def init(device: int = 0, use_torch_stream: bool = True) -> None:
    """Bind this process to a GPU.  With use_torch_stream the kernels run on
    torch's current stream, which orders them with torch.distributed
    collectives issued from the communication callbacks."""
    stream = None
    if use_torch_stream:
        import torch

        torch.cuda.set_device(device)
        stream = vp(torch.cuda.current_stream().cuda_stream)  # 0 = the default stream
    _H().call("fddh_init", device, stream, 0 if use_torch_stream else 1)


def set_print(on: bool) -> None:
    _H().call("fddh_set_print", int(on))


def comm_single() -> None:
    _H().call("fddh_comm_single")


def comm_rccl_from_torch() -> None:
    """RCCL called directly from the host layer; the 128-byte unique id is
    shipped through torch.distributed's store (no GPU traffic)."""
    import torch.distributed as dist

    rank, size = dist.get_rank(), dist.get_world_size()
    buf = ctypes.create_string_buffer(128)
    if rank == 0:
        _H().call("fddh_comm_rccl_unique_id", buf)
    obj = [bytes(buf.raw) if rank == 0 else None]
    dist.broadcast_object_list(obj, src=0)
    ident = ctypes.create_string_buffer(obj[0], 128)
    _H().call("fddh_comm_rccl_init", ident, rank, size)


def local_world(size: int):
    """Handle of an in-process world of `size` ranks (one host thread each, one shared GPU): see comm_local."""
    w = vp()
    _H().call("fddh_local_world_create", ctypes.byref(w), int(size))
    return w


def local_world_destroy(world) -> None:
    _H().call("fddh_local_world_destroy", world)


def comm_local(world, rank: int) -> None:
    """This THREAD becomes rank `rank` of the in-process world (call init(..., use_torch_stream=False) first: the
    rank's own stream).  Collectives are device-to-device copies / sums between the ranks' buffers."""
    _H().call("fddh_comm_local", world, int(rank))


def run_local_ranks(size: int, fn, device: int = 0, init_device: bool = True):
    """Run fn(rank, size) on `size` threads of this process, each bound to the GPU as one rank of a local world.
    Returns the list of results; the first exception of any rank is re-raised."""
    import threading

    # the ranks share this process's cores: each one's setup threads (host/host_parallel.hpp) take their share
    shared_cores = "FDD_HOST_THREADS" not in os.environ and size > 1
    if shared_cores:
        os.environ["FDD_HOST_THREADS"] = str(max(1, (os.cpu_count() or size) // size))
    world = local_world(size)
    results, errors = [None] * size, [None] * size

    def body(r):
        try:
            if init_device:
                init(device, use_torch_stream=False)
            set_print(False)
            comm_local(world, r)
            results[r] = fn(r, size)
        except BaseException as exc:  # noqa: BLE001 - reported to the caller below
            errors[r] = exc
            try:
                _H().call("fddh_local_world_fail", world)  # the peers waiting for this rank get an error now, not after the timeout
            except Exception:  # noqa: BLE001
                pass
        finally:
            try:
                _H().call("fddh_rank_finalize")  # the rank's own stream and communicator end with its thread
            except Exception:  # noqa: BLE001
                pass

    threads = [threading.Thread(target=body, args=(r,), name="fdd-rank-%d" % r) for r in range(size)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    local_world_destroy(world)
    if shared_cores:
        os.environ.pop("FDD_HOST_THREADS", None)
    first = [e for e in errors if e is not None and "a peer rank failed" not in str(e)] or [e for e in errors if e is not None]
    if first:
        raise first[0]  # the rank that failed first, not a peer's "a peer rank failed"
    return results


class _DevView:
    """Minimal __cuda_array_interface__ holder so torch can wrap a raw device pointer."""

    def __init__(self, ptr: int, shape, typestr: str):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2}


def comm_torch_callbacks(on_gpu: bool = True, staged: bool = False) -> None:
    """Collectives through torch.distributed (backend "nccl" = RCCL on GPUs,
    "gloo" on CPU buffers in the CPU test build).  staged: device buffers go
    through a host copy around the collective (a gloo group driving GPU ranks:
    the one-GPU rehearsal of the multi-rank path)."""
    import torch
    import torch.distributed as dist

    rank, size = dist.get_rank(), dist.get_world_size()

    views = {}  # (pointer, length, dtype) -> tensor view: the solve's exchange buffers are the same few on every call

    def wrap(ptr, n, dtype):
        key = (int(ptr or 0), int(n), dtype)
        t = views.get(key)
        if t is not None:
            return t
        if on_gpu:
            typestr = {torch.float64: "<f8", torch.uint8: "|u1"}[dtype]
            t = torch.as_tensor(_DevView(ptr, (n,), typestr), device="cuda")
        else:
            ctype = {torch.float64: ctypes.c_double, torch.uint8: ctypes.c_uint8}[dtype]
            t = torch.from_numpy(np.ctypeslib.as_array((ctype * n).from_address(ptr)))
        if len(views) < 4096:
            views[key] = t
        return t

    def allreduce(op):
        def fn(ctx, buf, n):
            try:
                t = wrap(buf, int(n), torch.float64)
                if staged:
                    h = t.cpu()
                    dist.all_reduce(h, op=op)
                    t.copy_(h)
                else:
                    dist.all_reduce(t, op=op)
                return 0
            except Exception as exc:  # pragma: no cover - surfaced by the C++ side
                print("allreduce callback failed:", exc, flush=True)
                return 1

        return fn

    def allgather(ctx, send, recv, nbytes):
        try:
            nbytes = int(nbytes)
            s = wrap(send, nbytes, torch.uint8)
            r = wrap(recv, nbytes * size, torch.uint8)
            if staged:
                hs = s.cpu()
                hr = [torch.empty_like(hs) for _ in range(size)]
                dist.all_gather(hr, hs)
                r.copy_(torch.cat(hr))
            elif on_gpu:
                dist.all_gather_into_tensor(r, s)
            else:
                dist.all_gather(list(r.chunk(size)), s)
            return 0
        except Exception as exc:  # pragma: no cover
            print("allgather callback failed:", exc, flush=True)
            return 1

    def barrier(ctx):
        try:
            dist.barrier()
            return 0
        except Exception as exc:  # pragma: no cover
            print("barrier callback failed:", exc, flush=True)
            return 1

    def exchange(ctx, n, peers, send, send_bytes, recv, recv_bytes):
        # the composite's ring pull: one message per peer and direction, all in flight together
        try:
            ops, staged_recv = [], []
            for i in range(int(n)):
                peer, ns, nr = int(peers[i]), int(send_bytes[i]), int(recv_bytes[i])
                if ns:
                    t = wrap(send[i], ns, torch.uint8)
                    ops.append(dist.P2POp(dist.isend, t.cpu() if staged else t, peer))
                if nr:
                    t = wrap(recv[i], nr, torch.uint8)
                    if staged:
                        h = torch.empty(nr, dtype=torch.uint8)
                        staged_recv.append((t, h))
                        t = h
                    ops.append(dist.P2POp(dist.irecv, t, peer))
            if ops:
                for req in dist.batch_isend_irecv(ops):
                    req.wait()
            for t, h in staged_recv:
                t.copy_(h)
            return 0
        except Exception as exc:  # pragma: no cover
            print("exchange callback failed:", exc, flush=True)
            return 1

    cbs = (_ALLREDUCE(allreduce(dist.ReduceOp.SUM)), _ALLREDUCE(allreduce(dist.ReduceOp.MAX)), _ALLGATHER(allgather), _BARRIER(barrier), _EXCHANGE(exchange))
    _keepalive.append(cbs)
    _H().call("fddh_comm_callbacks_ex", rank, size, None, *[ctypes.cast(c, vp) for c in cbs])


def rank_grid(num_ranks: int):
    """Same rule as the C++ driver: powers of two go round-robin over x, y, z."""
    P = [1, 1, 1]
    d = 0
    while num_ranks > 1 and num_ranks % 2 == 0:
        P[d] *= 2
        num_ranks //= 2
        d = (d + 1) % 3
    P[0] *= num_ranks
    return tuple(P)


def _arr3(v: Sequence[int]):
    return (ctypes.c_int * 3)(*[int(x) for x in v])


def _dp(a: Optional[np.ndarray]):
    if a is None:
        return vp(0)
    assert a.flags["C_CONTIGUOUS"]
    return vp(a.ctypes.data)


class Problem:
    """One rank's Domains (levels N, N-r, ..., 1) and optional Subdomain."""

    def __init__(self, handle):
        self.h = handle
        self.info = self._info()
        self.n = self.info["num_local_points"]

    @staticmethod
    def _flags(with_subdomain, block_local, force_composite):
        return (WITH_SUBDOMAIN if with_subdomain else 0) | (BLOCK_LOCAL if block_local else 0) | (FORCE_COMPOSITE if force_composite else 0)

    @classmethod
    def box(cls, E, P=(1, 1, 1), poly_degree=7, poly_reduction=2, with_subdomain=True, subdomain_overlap=1, superdomain_overlap=1, block_local=False, force_composite=False, faces="DDDDDD"):
        """With more than one rank the Subdomain is the full-domain-decomposition composite (own elements, rings at
        reduced degree, coarsened superdomain); block_local keeps the rank's own elements only.  faces: the boundary
        condition of x-, x+, y-, y+, z-, z+, 'D' Dirichlet (masked) or 'N' natural; see robin and boundary_rhs."""
        return cls.kershaw(E, P, poly_degree, poly_reduction, 1.0, with_subdomain, subdomain_overlap, superdomain_overlap, block_local, force_composite, faces=faces)

    @classmethod
    def kershaw(cls, E, P=(1, 1, 1), poly_degree=7, poly_reduction=2, eps=0.3, with_subdomain=True, subdomain_overlap=1, superdomain_overlap=1, block_local=False, force_composite=False, eps_z=None, faces="DDDDDD"):
        """The box under the generalized Kershaw map (the reference's experiment geometry, run.py:25-47: eps = 0.3); all
        six geometric factors are non-zero.  eps = 1 is the uniform box.  faces: as in box (the map keeps the faces)."""
        h = vp()
        _H().call("fddh_problem_create_box_faces", ctypes.byref(h), _arr3(E), _arr3(P), poly_degree, poly_reduction, subdomain_overlap, superdomain_overlap,
                  cls._flags(with_subdomain, block_local, force_composite), ctypes.c_double(eps), ctypes.c_double(eps if eps_z is None else eps_z), str(faces).encode())
        return cls(h)

    @classmethod
    def from_directory(cls, directory, poly_degree, poly_reduction, subdomain_overlap=1, superdomain_overlap=1, with_subdomain=True, block_local=False, force_composite=False):
        h = vp()
        _H().call("fddh_problem_create_dir_ex", ctypes.byref(h), os.fsencode(directory), poly_degree, poly_reduction, subdomain_overlap, superdomain_overlap, cls._flags(with_subdomain, block_local, force_composite))
        return cls(h)

    def sub_info(self):
        buf = (ctypes.c_longlong * len(SUB_INFO_NAMES))()
        _H().call("fddh_problem_sub_info", self.h, buf, len(SUB_INFO_NAMES))
        return {k: int(buf[i]) for i, k in enumerate(SUB_INFO_NAMES)}

    def sub_region(self):
        n = self.sub_info()["num_ext_elems"]
        ids, lv = np.zeros(n, np.int32), np.zeros(n, np.int32)
        ip = ctypes.POINTER(ctypes.c_int)
        _H().call("fddh_problem_sub_region", self.h, ids.ctypes.data_as(ip), lv.ctypes.data_as(ip), n)
        return ids, lv

    def sub_composite_levels(self):
        kept = np.zeros(32, np.int32)
        nl = ctypes.c_int()
        _H().call("fddh_problem_sub_composite_levels", self.h, kept.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 32, ctypes.byref(nl))
        return [int(k) for k in kept[: nl.value]]

    def close(self):
        if self.h:
            _H().call("fddh_problem_destroy", self.h)
            self.h = None

    def _info(self):
        buf = (ctypes.c_longlong * len(INFO_NAMES))()
        _H().call("fddh_problem_info", self.h, buf, len(INFO_NAMES))
        return {k: int(buf[i]) for i, k in enumerate(INFO_NAMES)}

    def refresh(self):
        self.info = self._info()
        return self.info

    def level_degree(self, level):
        d = ctypes.c_int()
        _H().call("fddh_problem_level_degree", self.h, level, ctypes.byref(d))
        return d.value

    def mesh_array(self, name, level=0):
        deg = self.level_degree(level)
        npts = self.info["num_local_elements"] * (deg + 1) ** self.info["dim"]
        if name == "z" and self.info["dim"] == 2:
            return np.zeros(npts)  # a 2-D mesh has no z file (domain.tpp:121-138)
        dtype = {"glo_num": np.int64, "node_degree": np.int32}.get(name, np.float64)
        out = np.zeros(npts, dtype)
        _H().call("fddh_problem_mesh_array", self.h, level, name.encode(), _dp(out), out.nbytes)
        return out

    def csr(self, which):
        nr, nc, nz = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _H().call("fddh_problem_csr", self.h, which, ctypes.byref(nr), ctypes.byref(nc), ctypes.byref(nz), None, None, None)
        ptr = np.zeros(nr.value + 1, np.int32)
        col = np.zeros(nz.value, np.int32)
        val = np.zeros(nz.value)
        _H().call("fddh_problem_csr", self.h, which, None, None, None, _dp(ptr), _dp(col), _dp(val))
        return (nr.value, nc.value), ptr, col, val

    def assembled_weight(self):
        out = np.zeros(self.info["num_local_nodes"])
        _H().call("fddh_problem_assembled_weight", self.h, _dp(out), len(out))
        return out

    def set_D_hat(self, level, D):
        D = np.ascontiguousarray(D, dtype=np.float64)
        n = self.level_degree(level) + 1
        _H().call("fddh_problem_set_D_hat", self.h, level, _dp(D), n)

    def get_D_hat(self, level):
        n = self.level_degree(level) + 1
        D = np.zeros(n * n)
        _H().call("fddh_problem_get_D_hat", self.h, level, _dp(D), n)
        return D

    def set_options(self, max_iterations=-1, tolerance=float("nan"), num_vectors=-1, use_preconditioner=-1, preconditioner_type=-1, sub_num_vectors=-1, sub_max_iterations=-1, sub_build_tree=-1):
        _H().call("fddh_problem_set_options", self.h, max_iterations, tolerance, num_vectors, int(use_preconditioner), preconditioner_type, sub_num_vectors, sub_max_iterations, int(sub_build_tree))

    def set_flag(self, name, value):
        _H().call("fddh_problem_set_flag", self.h, name.encode(), int(value))

    def affine_info(self):
        """after set_flag("affine_geometry", 1): which operators run without streaming the factor arrays (an option of
        this build) and how far the mesh's own factors are from the form c_f(e) (w_i w_j) w_k"""
        dom, aff, lists, dev = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_double(-1.0)
        _H().call("fddh_problem_affine_info", self.h, ctypes.byref(dom), ctypes.byref(aff), ctypes.byref(lists), ctypes.byref(dev))
        return {"fine_domain": bool(dom.value), "sub_lists_affine": aff.value, "sub_lists": lists.value, "max_deviation": dev.value}

    def zero_factor_info(self):
        """flag "skip_zero_factors": is it on, does the fine domain's list run the kernel that streams three factor arrays
        (its three off-diagonal arrays are zero at every point), and how many of the subdomain's lists do, of how many"""
        on, dom, diag, lists = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        _H().call("fddh_problem_zero_factor_info", self.h, ctypes.byref(on), ctypes.byref(dom), ctypes.byref(diag), ctypes.byref(lists))
        return {"enabled": bool(on.value), "fine_domain": bool(dom.value), "sub_lists_diag": diag.value, "sub_lists": lists.value}

    def mfma_zero_factor_info(self):
        """flag "mfma_skip_zero_factors": is it on, does the fine domain's list run the matrix-core kernel that streams three
        factor arrays (degree 11..15, off-diagonal arrays zero at every point), and how many of the subdomain's lists do, of
        how many"""
        on, dom, diag, lists = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        _H().call("fddh_problem_mfma_zero_factor_info", self.h, ctypes.byref(on), ctypes.byref(dom), ctypes.byref(diag), ctypes.byref(lists))
        return {"enabled": bool(on.value), "fine_domain": bool(dom.value), "sub_lists_mfma_diag": diag.value, "sub_lists": lists.value}

    def line_stiffness_info(self):
        """flag "line_stiffness": is it on, does the fine domain's list run the line form of the three-array stiffness
        kernel (degree 7), and how many of the subdomain's lists do, of how many"""
        on, dom, lines, lists = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        _H().call("fddh_problem_line_stiffness_info", self.h, ctypes.byref(on), ctypes.byref(dom), ctypes.byref(lines), ctypes.byref(lists))
        return {"enabled": bool(on.value), "fine_domain": bool(dom.value), "sub_lists_lines": lines.value, "sub_lists": lists.value}

    def shared_factor_info(self):
        """flag "shared_factor_blocks": is it on, does the fine domain's list run the line kernel's shared instance (its
        elements hold the factor blocks of a few of them, bit for bit) and how many distinct blocks were found there, and
        how many of the subdomain's lists run it, of how many"""
        on, dom, classes, shared, lists = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        _H().call("fddh_problem_shared_factor_info", self.h, ctypes.byref(on), ctypes.byref(dom), ctypes.byref(classes), ctypes.byref(shared), ctypes.byref(lists))
        return {"enabled": bool(on.value), "fine_domain": bool(dom.value), "fine_domain_classes": classes.value, "sub_lists_shared": shared.value, "sub_lists": lists.value}

    def lean_line_info(self):
        """flag "lean_line_stiffness": is it on, does the fine domain's uploaded D_hat meet the lean line instance's
        conditions (zero interior diagonal, negated mirror image bit for bit), does its list run that instance, and how
        many of the subdomain's lists do, of how many"""
        on, ok, dom, lean, lists = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        _H().call("fddh_problem_lean_line_info", self.h, ctypes.byref(on), ctypes.byref(ok), ctypes.byref(dom), ctypes.byref(lean), ctypes.byref(lists))
        return {"enabled": bool(on.value), "fine_domain_table_ok": bool(ok.value), "fine_domain": bool(dom.value), "sub_lists_lean": lean.value, "sub_lists": lists.value}

    def assembly_info(self):
        """flag "assemble_in_stiffness": is it on, is it in effect in the subdomain's dof-space operator (and why not),
        Qt's rows and the region's points by class, the row blocks of the general rows' plan"""
        on, eff, blocks = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        rows, points, why = (ctypes.c_longlong * 3)(), (ctypes.c_longlong * 5)(), ctypes.create_string_buffer(256)
        _H().call("fddh_problem_assembly_info", self.h, ctypes.byref(on), ctypes.byref(eff), rows, points, ctypes.byref(blocks), why, len(why))
        return {"enabled": bool(on.value), "in_effect": bool(eff.value), "why_not": why.value.decode(), "rows": dict(zip(("general", "single", "pair"), map(int, rows))),
                "points": dict(zip(("general", "single", "pair_low", "pair_high", "none"), map(int, points))), "reduced_row_blocks": blocks.value}

    def assembly_arrays(self):
        """(point_class_dof, ptr, col, row_map): point_dof with the class of each point in bits 29..30, and the general rows
        of Qt as a CSR of their own with their dofs"""
        npts, nr, nz = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _H().call("fddh_problem_assembly_arrays", self.h, ctypes.byref(npts), ctypes.byref(nr), ctypes.byref(nz), None, None, None, None)
        pcd, ptr, col, rmap = np.zeros(npts.value, np.int32), np.zeros(nr.value + 1, np.int32), np.zeros(nz.value, np.int32), np.zeros(nr.value, np.int32)
        ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        _H().call("fddh_problem_assembly_arrays", self.h, None, None, None, ip(pcd), ip(ptr), ip(col), ip(rmap))
        return pcd, ptr, col, rmap

    def dssum(self, u, mask=True, weight=False):
        out = np.zeros(self.n)
        _H().call("fddh_problem_dssum", self.h, _dp(out), _dp(np.ascontiguousarray(u)), int(mask), int(weight))
        return out

    def stiffness(self, u, dssum=False):
        out = np.zeros(self.n)
        _H().call("fddh_problem_stiffness", self.h, _dp(out), _dp(np.ascontiguousarray(u)), int(dssum))
        return out

    def mass(self):
        """The diagonal mass matrix B = w_i w_j w_k det J at the fine level's points, unassembled.  The right-hand side of
        -laplace(u) = s from the source term s at the points:

            f = p.mass() * s
            u, its, hist = p.solve(f)
        """
        out = np.zeros(self.n)
        _H().call("fddh_field_mass", self.h, _dp(out))
        return out

    def gradient(self, u, average=False):
        """(gx, gy, gz): the gradient of u, per element; average: each component replaced by its multiplicity-weighted
        mean over the copies of a node (continuous; collective on several ranks)"""
        g = [np.zeros(self.n) for _ in range(3)]
        _H().call("fddh_field_gradient", self.h, _dp(np.ascontiguousarray(u, dtype=np.float64)), _dp(g[0]), _dp(g[1]), _dp(g[2]), int(average))
        return tuple(g)

    def weak_divergence(self, vx, vy, vz):
        """out_i = integral of grad(phi_i) . v, unassembled like the f of make_rhs: weak_divergence(*gradient(u)) is
        stiffness(u)"""
        out = np.zeros(self.n)
        v = [np.ascontiguousarray(c, dtype=np.float64) for c in (vx, vy, vz)]
        _H().call("fddh_field_weak_divergence", self.h, _dp(v[0]), _dp(v[1]), _dp(v[2]), _dp(out))
        return out

    def _convect(self, entry, cx, cy, cz, u):
        out = np.zeros(self.n)
        v = [np.ascontiguousarray(c, dtype=np.float64) for c in (cx, cy, cz, u)]
        _H().call(entry, self.h, _dp(v[0]), _dp(v[1]), _dp(v[2]), _dp(v[3]), _dp(out))
        return out

    def convect(self, cx, cy, cz, u):
        """c . grad u at every point (collocated), per element"""
        return self._convect("fddh_convect", cx, cy, cz, u)

    def weak_convect(self, cx, cy, cz, u):
        """out_i = integral of phi_i (c . grad u) on the (3n+1)/2 Gauss-Legendre points per direction (the 3/2 rule),
        unassembled like weak_divergence: dssum(p.weak_convect(cx, cy, cz, u)) is the convection term of a weak form"""
        return self._convect("fddh_weak_convect", cx, cy, cz, u)

    def quadrature(self):
        """(z, w, P, Pd) of weak_convect's rule: M Gauss-Legendre points and weights, P[q, i] = l_i(z_q) and Pd = P D_hat"""
        M = ctypes.c_int(0)
        _H().call("fddh_convect_quadrature", self.h, ctypes.byref(M), None, None, None, None)
        n = self.level_degree(0) + 1
        z, w, P, Pd = np.zeros(M.value), np.zeros(M.value), np.zeros((M.value, n)), np.zeros((M.value, n))
        _H().call("fddh_convect_quadrature", self.h, None, _dp(z), _dp(w), _dp(P), _dp(Pd))
        return z, w, P, Pd

    # --- Helmholtz solves (an addition of this build, include/fdd_host.h) ---
    def helmholtz(self, lam):
        """Solve (-laplace + lam) u = f from here on: lam a constant >= 0 or an array >= 0 over the fine level's points; 0
        switches the term off.  One rank, conforming region, 3-D.  A manufactured right-hand side:

            f = p.stiffness(u_star) + lam * p.mass() * u_star
        """
        if np.ndim(lam) == 0:
            _H().call("fddh_helmholtz_set", self.h, ctypes.c_double(float(lam)), None)
        else:
            lam = np.ascontiguousarray(lam, dtype=np.float64)
            if lam.shape != (self.n,):
                raise ValueError("lam has one value per point of the fine level (%d), got shape %s" % (self.n, lam.shape))
            _H().call("fddh_helmholtz_set", self.h, ctypes.c_double(0.0), _dp(lam))

    def helmholtz_info(self):
        """{"active", "min", "max"}: whether a shift is set and the range of the lam it was made from"""
        on, lo, hi = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
        _H().call("fddh_helmholtz_info", self.h, ctypes.byref(on), ctypes.byref(lo), ctypes.byref(hi))
        return {"active": bool(on.value), "min": lo.value, "max": hi.value}

    def helmholtz_shift(self):
        """cbar on the rank's nodes: the sums of lam * mass() over the copies of every node (zeros when no shift is set)"""
        out = np.zeros(self.info["num_local_nodes"])
        _H().call("fddh_helmholtz_shift", self.h, _dp(out), len(out))
        return out

    def helmholtz_node_operator(self, v):
        """(q, <v, q>) with q = (Qt A_L Q + diag(cbar)) v on node vectors: the outer step's operator application and its dot"""
        v = np.ascontiguousarray(v, dtype=np.float64)
        q = np.zeros(len(v))
        vq = ctypes.c_double()
        _H().call("fddh_helmholtz_node_operator", self.h, _dp(v), _dp(q), len(v), ctypes.byref(vq))
        return q, vq.value

    def inner_norm_counters(self):
        """{"estimated", "exact", "min_ratio"}: over the life of the problem's Subdomain, the last Arnoldi steps of inner GMRES
        cycles that took their norm from the projections (flag "last_norm_from_projections"), those that ran the exact pass
        instead, and the smallest (<q, q> - sum h^2) / <q, q> among them (0.0 before the first)"""
        est, exact, ratio = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_double()
        _H().call("fddh_inner_norm_counters", self.h, ctypes.byref(est), ctypes.byref(exact), ctypes.byref(ratio))
        return {"estimated": est.value, "exact": exact.value, "min_ratio": ratio.value}

    # --- Neumann and Robin faces (an addition of this build, include/fdd_host.h) ---
    def boundary_info(self):
        """{"faces", "num_faces", "robin_active", "alpha_min", "alpha_max", "shift_support", "indexed_shift",
        "indexed_outer", "indexed_inner"}: the face codes ("" and -1 faces for a problem made from files), the range of a
        set Robin coefficient, the non-zero entries of the node shift and which shift kernel the operators run"""
        codes = ctypes.create_string_buffer(7)
        m, on, flag, use = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        lo, hi, support = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
        _H().call("fddh_boundary_info", self.h, codes, ctypes.byref(m), ctypes.byref(on), ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(support), ctypes.byref(flag), ctypes.byref(use))
        return {"faces": codes.value.decode(), "num_faces": m.value, "robin_active": bool(on.value), "alpha_min": lo.value, "alpha_max": hi.value, "shift_support": support.value,
                "indexed_shift": bool(flag.value), "indexed_outer": bool(use.value & 1), "indexed_inner": bool(use.value & 2)}

    def surface(self, normal=True):
        """The faces of the rank's elements on the surface of the box, sorted by (side, element): {"elem", "side"} (m each;
        side = 2 axis + upper), "points" (m, n, n): the index of every face point in a point vector, [f, b, a] with (a, b) =
        (j, k) on x-faces, (i, k) on y-faces, (i, j) on z-faces, "area" (m, n, n): the weight of the surface integral, and
        "normal" (3, m, n, n): the unit outward normal (None with normal=False).  The integral of g over the surface is
        (area * g[points]).sum(); the flux du/dn is sum_a normal[a] * gradient(u)[a][points]."""
        m, n = self.boundary_info()["num_faces"], self.level_degree(0) + 1
        elem, side = np.zeros(max(m, 0), np.int32), np.zeros(max(m, 0), np.int32)
        ip = ctypes.POINTER(ctypes.c_int)
        _H().call("fddh_boundary_faces", self.h, elem.ctypes.data_as(ip), side.ctypes.data_as(ip), m)
        area = np.zeros((m, n, n))
        nrm = np.zeros((3, m, n, n)) if normal else None
        _H().call("fddh_boundary_surface", self.h, _dp(area), *([_dp(nrm[a]) for a in range(3)] if normal else [None] * 3), ctypes.c_longlong(area.size))
        b, a = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        fixed = np.where(side % 2 == 1, n - 1, 0)[:, None, None]
        axis = (side // 2)[:, None, None]
        in_elem = np.where(axis == 0, fixed + n * (a + n * b), np.where(axis == 1, a + n * (fixed + n * b), a + n * (b + n * fixed)))
        return {"elem": elem, "side": side, "points": elem.astype(np.int64)[:, None, None] * n**3 + in_elem, "area": area, "normal": nrm}

    def robin(self, alpha):
        """The condition kappa du/dn + alpha u = g on natural faces from here on: alpha None (clears), {side: value} (a
        constant on every face of those sides, 0 elsewhere; masked points -- the edges shared with a 'D' face -- are left
        at 0) or an (m, n, n) array over surface()["points"], >= 0 and 0 on masked points.  One rank, conforming region.
        The datum g enters the right-hand side as a flux (boundary_rhs)."""
        if alpha is None:
            _H().call("fddh_boundary_robin_set", self.h, None)
            return
        if isinstance(alpha, dict):
            s = self.surface(normal=False)
            free = self.mesh_array("p_mask")[s["points"]] != 0.0
            values = np.zeros(s["area"].shape)
            for side, value in alpha.items():
                if int(side) not in range(6):
                    raise ValueError("a side is 0..5 (x-, x+, y-, y+, z-, z+), got %r" % (side,))
                values[s["side"] == int(side)] = float(value)
            alpha = values * free
        alpha = np.ascontiguousarray(alpha, dtype=np.float64)
        m, n = self.boundary_info()["num_faces"], self.level_degree(0) + 1
        if alpha.shape != (m, n, n):
            raise ValueError("alpha has one value per face point, shape %s, got %s" % ((m, n, n), alpha.shape))
        _H().call("fddh_boundary_robin_set", self.h, _dp(alpha))

    def boundary_rhs(self, f, dirichlet=None, flux=None, lam=0.0):
        """The right-hand side of a problem with boundary data, f' = f - A_L u_D - lam * B * u_D + scatter(area * flux):
          dirichlet  the prescribed values, an array over the points (read at the masked points only) or a scalar; u_D is
                     that on the masked points and 0 elsewhere
          flux       the natural datum per face point, (m, n, n) over surface()["points"]: the Neumann datum or the g of a
                     Robin condition.  Under a diffusivity it is kappa du/dn, not du/dn
          lam        the lam handed to helmholtz()
        A_L is stiffness(), so a set diffusivity is followed.  The solution is solve(f')[0] + u_D, u_D formed by the caller
        as here (the solve leaves the masked points at 0).  Numpy on the host:
        the data are formed once per right-hand side."""
        out = np.array(f, dtype=np.float64, copy=True)
        u_D = np.zeros(self.n)
        if dirichlet is not None:
            masked = self.mesh_array("p_mask") == 0.0
            u_D[masked] = np.broadcast_to(np.asarray(dirichlet, dtype=np.float64), (self.n,))[masked]
            out -= self.stiffness(u_D)
            if np.any(np.asarray(lam) != 0.0):
                out -= lam * self.mass() * u_D
        if flux is not None:
            s = self.surface(normal=False)
            flux = np.asarray(flux, dtype=np.float64)
            if flux.shape != s["area"].shape:
                raise ValueError("flux has one value per face point, shape %s, got %s" % (s["area"].shape, flux.shape))
            np.add.at(out, s["points"].reshape(-1), (s["area"] * flux).reshape(-1))
        return out

    # --- variable diffusivity (an addition of this build, include/fdd_host.h) ---
    def diffusivity(self, kappa):
        """Solve -div(kappa grad u) (+ lam u) = f from here on: kappa > 0 a scalar (broadcast) or an array over the fine
        level's points, element-major like mesh_array("x"); None clears.  One rank, conforming region, 3-D.  stiffness,
        make_rhs_from, the solves, the inner operator and its diagonal and amg_build follow; mass, gradient and
        weak_divergence are geometry and do not."""
        if kappa is None:
            _H().call("fddh_diffusivity_set", self.h, None, 0)
            return
        if np.ndim(kappa) == 0:
            kappa = np.full(self.n, float(kappa))
        kappa = np.ascontiguousarray(kappa, dtype=np.float64)
        if kappa.ndim != 1:
            raise ValueError("kappa has one value per point of the fine level (%d), got shape %s" % (self.n, kappa.shape))
        _H().call("fddh_diffusivity_set", self.h, _dp(kappa), len(kappa))

    def diffusivity_info(self):
        """{"active", "min", "max"}: whether a kappa is set and its range; flag "coefficient_in_kernel": does the fine
        domain's list run the coefficient instance of the line kernel, and how many of the subdomain's lists do, of how many"""
        on, lo, hi = ctypes.c_int(0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        dom, inside, lists = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        _H().call("fddh_diffusivity_info", self.h, ctypes.byref(on), ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(dom), ctypes.byref(inside), ctypes.byref(lists))
        return {"active": bool(on.value), "min": lo.value, "max": hi.value, "fine_domain_in_kernel": bool(dom.value), "sub_lists_in_kernel": inside.value, "sub_lists": lists.value}

    def residual_norm(self, r):
        v = ctypes.c_double()
        _H().call("fddh_problem_residual_norm", self.h, _dp(np.ascontiguousarray(r)), ctypes.byref(v))
        return v.value

    def make_rhs(self, function_id=0, seed=0):
        u_star, f = np.zeros(self.n), np.zeros(self.n)
        _H().call("fddh_problem_make_rhs", self.h, function_id, seed, _dp(u_star), _dp(f))
        return u_star, f

    def make_rhs_from(self, u_star):
        u_star = np.ascontiguousarray(u_star, dtype=np.float64).copy()
        f = np.zeros(self.n)
        _H().call("fddh_problem_make_rhs_from", self.h, _dp(u_star), _dp(f))
        return u_star, f

    def solve(self, f, method="fcg"):
        u = np.zeros(self.n)
        cap = 4096
        hist = np.zeros(cap)
        nh, its = ctypes.c_int(), ctypes.c_int()
        _H().call("fddh_problem_solve", self.h, 0 if method == "fcg" else 1, _dp(np.ascontiguousarray(f)), _dp(u), _dp(hist), cap, ctypes.byref(nh), ctypes.byref(its))
        return u, its.value, hist[: min(nh.value, cap)].copy()

    def solve_timed(self, f, method="fcg", want_solution=False):
        """(iterations, history, seconds): the solve with the clock around the device work only"""
        u = np.zeros(self.n) if want_solution else None
        cap = 4096
        hist = np.zeros(cap)
        nh, its, sec = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
        _H().call("fddh_problem_solve_timed", self.h, 0 if method == "fcg" else 1, _dp(np.ascontiguousarray(f)), _dp(u), _dp(hist), cap, ctypes.byref(nh), ctypes.byref(its), ctypes.byref(sec))
        return its.value, hist[: min(nh.value, cap)].copy(), sec.value

    # --- successive-right-hand-side projection (an addition of this build, include/fdd_host.h) ---
    def projection(self, capacity):
        """Keep up to `capacity` (1..16) earlier solutions as a start-value basis for solve_projected; 0 switches it off."""
        _H().call("fddh_problem_projection_configure", self.h, int(capacity))

    def projection_clear(self):
        _H().call("fddh_problem_projection_clear", self.h)

    def projection_info(self):
        cap, size, restarts = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
        _H().call("fddh_problem_projection_info", self.h, ctypes.byref(cap), ctypes.byref(size), ctypes.byref(restarts))
        return {"capacity": cap.value, "size": size.value, "restarts": restarts.value}

    def projection_basis(self, k):
        """(X_k, A_L X_k) of the basis, k < size"""
        x, ax = np.zeros(self.n), np.zeros(self.n)
        _H().call("fddh_problem_projection_basis", self.h, int(k), _dp(x), _dp(ax))
        return x, ax

    def solve_projected(self, f, method="fcg", timed=False):
        """(u, iterations, history, proj): solve() started from the projection of f onto the basis, which then takes the
        correction in.  proj = [|f|, |f - A x0|, basis size used, basis size afterwards] and, timed, a fifth entry: the
        device seconds as solve_timed takes them, the projection included."""
        u = np.zeros(self.n)
        cap = 4096
        hist = np.zeros(cap)
        nh, its, sec = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
        proj = np.zeros(4)
        _H().call("fddh_problem_solve_projected", self.h, 0 if method == "fcg" else 1, _dp(np.ascontiguousarray(f, dtype=np.float64)), _dp(u), _dp(hist), cap, ctypes.byref(nh), ctypes.byref(its), _dp(proj),
                  ctypes.byref(sec) if timed else None)
        if timed:
            proj = np.append(proj, sec.value)
        return u, its.value, hist[: min(nh.value, cap)].copy(), proj

    def precond_apply(self, r, method="gmres"):
        z = np.zeros(self.n)
        hist = np.zeros(64)
        nh = ctypes.c_int()
        _H().call("fddh_problem_precond_apply", self.h, 0 if method == "fcg" else 1, _dp(np.ascontiguousarray(r)), _dp(z), _dp(hist), 64, ctypes.byref(nh))
        return z, hist[: nh.value].copy()

    def comm_time(self, iterations=20):
        """the solve path's collectives alone (collective call): dict name -> (avg us, bytes)"""
        us = (ctypes.c_double * 6)()
        nbytes = (ctypes.c_double * 6)()
        _H().call("fddh_problem_comm_time", self.h, int(iterations), us, nbytes)
        # the last two are what the solve issues by default (point-to-point groups: xGMI links every pair of GPUs directly);
        # the dense all-reduce / all-gather forms before them are the flags' other setting, timed for comparison
        names = ["allreduce_3_scalars", "interface_pair_allreduce", "coarse_allgather", "ring_exchange", "interface_pair_neighbour_exchange", "ring_and_coarse_exchange"]
        return {n: {"avg_us": us[k], "bytes": nbytes[k]} for k, n in enumerate(names)}

    def sub_op(self, op, u):
        code = {"tree": 0, "stiffness": 1, "dssum": 2}[op]
        out = np.zeros(self.info["sub_num_values"])
        _H().call("fddh_problem_sub_op", self.h, code, _dp(np.ascontiguousarray(u)), _dp(out))
        return out

    def sub_dof_operator(self, x):
        """y = (Qt A_L Q | A_sup) x on the unique dofs of the inner iteration"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros(len(x))
        _H().call("fddh_problem_sub_dof_op", self.h, 0, _dp(x), _dp(y), len(x))
        return y

    def sub_jacobi_diagonal(self):
        n = self.sub_info()["unique_dofs"]
        d = np.zeros(n)
        _H().call("fddh_problem_sub_jacobi_diagonal", self.h, _dp(d), n)
        return d

    def sub_dof_solve(self, fa):
        """ua = the configured inner solve (GMRES(m), or Chebyshev-Jacobi with the flag "inner_solver" = 1) of the dof-space
        right-hand side fa, from a zero start"""
        fa = np.ascontiguousarray(fa, dtype=np.float64)
        ua = np.zeros(len(fa))
        _H().call("fddh_problem_sub_dof_solve", self.h, _dp(fa), _dp(ua), len(fa))
        return ua

    # --- Chebyshev-Jacobi inner solve (an addition of this build, include/fdd_host.h) ---
    def inner_chebyshev(self, order=None, lower=None, upper=None, power_iterations=None):
        """Settings of the Chebyshev-Jacobi inner solve (switched on by set_flag("inner_solver", 1)); None keeps a value."""
        o, lo, up, it = ctypes.c_int(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        _H().call("fddh_problem_inner_chebyshev_info", self.h, ctypes.byref(o), ctypes.byref(lo), ctypes.byref(up), None, ctypes.byref(it))
        _H().call("fddh_problem_inner_chebyshev_configure", self.h, int(o.value if order is None else order), ctypes.c_double(lo.value if lower is None else lower),
                  ctypes.c_double(up.value if upper is None else upper), int(it.value if power_iterations is None else power_iterations))

    def inner_chebyshev_info(self):
        """{"order", "lower", "upper", "lambda", "power_iterations"}; lambda is computed now if it is not cached"""
        o, lo, up, lam, it = ctypes.c_int(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        _H().call("fddh_problem_inner_chebyshev_info", self.h, ctypes.byref(o), ctypes.byref(lo), ctypes.byref(up), ctypes.byref(lam), ctypes.byref(it))
        return {"order": o.value, "lower": lo.value, "upper": up.value, "lambda": lam.value, "power_iterations": it.value}

    def sub_dof_rhs(self, r):
        """the dof-space right-hand side of the inner solve for the outer point vector r (collective on a composite)"""
        n = self.sub_info()["unique_dofs"]
        y = np.zeros(n)
        _H().call("fddh_problem_sub_dof_op", self.h, 1, _dp(np.ascontiguousarray(r, dtype=np.float64)), _dp(y), n)
        return y

    # --- low-order AMG preconditioner of the inner solve (hierarchy handed in) ---
    def sub_point_dofs(self):
        n = self.sub_info()["num_points"]
        dof = np.zeros(n, dtype=np.int32)
        _H().call("fddh_problem_sub_point_dofs", self.h, dof.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n)
        return dof

    def amg_attach(self, levels):
        """levels: finest first, dicts with A (scipy CSR), D (diagonal scaling),
        coefs (Chebyshev coefficients) and P (scipy CSR, None on the coarsest)."""
        ip = ctypes.POINTER(ctypes.c_int)
        for lv in levels:
            A = lv["A"].tocsr()
            A.sort_indices()
            a = (np.ascontiguousarray(A.indptr, dtype=np.int32), np.ascontiguousarray(A.indices, dtype=np.int32), np.ascontiguousarray(A.data, dtype=np.float64))
            D = np.ascontiguousarray(lv["D"], dtype=np.float64)
            coefs = np.ascontiguousarray(lv["coefs"], dtype=np.float64)
            if lv.get("P") is not None:
                P = lv["P"].tocsr()
                P.sort_indices()
                pp = (np.ascontiguousarray(P.indptr, dtype=np.int32), np.ascontiguousarray(P.indices, dtype=np.int32), np.ascontiguousarray(P.data, dtype=np.float64))
                pargs = (P.shape[1], pp[0].ctypes.data_as(ip), pp[1].ctypes.data_as(ip), _dp(pp[2]))
            else:
                pargs = (0, None, None, None)
            _H().call("fddh_problem_amg_add_level", self.h, A.shape[0], a[0].ctypes.data_as(ip), a[1].ctypes.data_as(ip), _dp(a[2]), _dp(D), _dp(coefs), len(coefs), *pargs)
        _H().call("fddh_problem_amg_finalize", self.h)

    def amg_build(self, coarsest_size=0, strength=0.0, smooth_prolongator=True, verbose=False, device=None):
        """Low-order FEM matrix + smoothed-aggregation hierarchy built by the host layer; returns the level count.
        device: None leaves the flag "amg_device_setup" as it is, True / False sets it first (the leading levels on the GPU)."""
        if device is not None:
            self.set_flag("amg_device_setup", 1 if device else 0)
        nl = ctypes.c_int()
        _H().call("fddh_problem_amg_build", self.h, int(coarsest_size), float(strength), int(smooth_prolongator), int(verbose), ctypes.byref(nl))
        return nl.value

    def amg_setup_info(self):
        """The last hierarchy build: {"levels_built_on_device": int, "setup_seconds": float} (0 levels: a host build)."""
        lv, sec = ctypes.c_int(0), ctypes.c_double(0.0)
        _H().call("fddh_problem_amg_setup_info", self.h, ctypes.byref(lv), ctypes.byref(sec))
        return {"levels_built_on_device": lv.value, "setup_seconds": sec.value}

    def amg_level_transfer(self, level):
        """True where the interpolator of `level` is applied matrix-free (fdd_lattice_prolong / _restrict)."""
        flag = ctypes.c_int(0)
        _H().call("fddh_problem_amg_level_transfer", self.h, int(level), ctypes.byref(flag))
        return bool(flag.value)

    def amg_levels(self, cheby_order=2):
        """The attached hierarchy as scipy matrices (finest first), as amg_attach takes it."""
        import scipy.sparse as sp

        ip = ctypes.POINTER(ctypes.c_int)
        out = []
        level = 0
        while True:
            n, nnz, nc, nnzp = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            try:
                _H().call("fddh_problem_amg_level_info", self.h, level, ctypes.byref(n), ctypes.byref(nnz), ctypes.byref(nc), ctypes.byref(nnzp))
            except lib.FddError:
                break
            ap, ac, av = np.zeros(n.value + 1, np.int32), np.zeros(nnz.value, np.int32), np.zeros(nnz.value)
            D, coefs = np.zeros(n.value), np.zeros(8)
            has_p = nnzp.value > 0
            pp, pc, pv = np.zeros(n.value + 1, np.int32), np.zeros(max(nnzp.value, 1), np.int32), np.zeros(max(nnzp.value, 1))
            _H().call("fddh_problem_amg_level_arrays", self.h, level, ap.ctypes.data_as(ip), ac.ctypes.data_as(ip), _dp(av), _dp(D), _dp(coefs),
                      pp.ctypes.data_as(ip) if has_p else None, pc.ctypes.data_as(ip) if has_p else None, _dp(pv) if has_p else None)
            lv = {"A": sp.csr_matrix((av, ac, ap), shape=(n.value, n.value)), "D": D, "coefs": coefs[:cheby_order].copy(), "P": None}
            if has_p:
                lv["P"] = sp.csr_matrix((pv[: nnzp.value], pc[: nnzp.value], pp), shape=(n.value, nc.value))
            out.append(lv)
            level += 1
        return out

    def amg_apply(self, r):
        z = np.zeros(self.n)
        _H().call("fddh_problem_amg_apply", self.h, _dp(np.ascontiguousarray(r)), _dp(z))
        return z

    def sub_residual_norm(self, r):
        v = ctypes.c_double()
        _H().call("fddh_problem_sub_residual_norm", self.h, _dp(np.ascontiguousarray(r)), ctypes.byref(v))
        return v.value

    def pcg_begin(self, f):
        _H().call("fddh_problem_pcg_begin", self.h, _dp(np.ascontiguousarray(f)))

    def pcg_steps(self, steps):
        v = ctypes.c_double()
        _H().call("fddh_problem_pcg_steps", self.h, steps, ctypes.byref(v))
        return v.value

    def pcg_solution(self):
        u = np.zeros(self.n)
        _H().call("fddh_problem_pcg_solution", self.h, _dp(u))
        return u


def spmv_stencil_time(m, iterations=10):
    """(avg_us, algorithmic_bytes, nnz) of the 27-point-stencil SpMV on an m^3 node grid"""
    us, nbytes, nnz = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
    _H().call("fddh_spmv_stencil_time", int(m), int(iterations), ctypes.byref(us), ctypes.byref(nbytes), ctypes.byref(nnz))
    return us.value, nbytes.value, nnz.value


def sync():
    _H().call("fddh_sync")


def barrier():
    _H().call("fddh_barrier")
