"""ctypes driver for the host emulation of the bounded least-squares solver and of the two kernels that end in it
(tests/emu_bvls/emu_bvls.cpp, compiled on demand with g++ from trep_amd/csrc/bvls_solve.hpp, lsq_solve.hpp, mvi_dyn_inverse.hpp and
mvi_inverse.hpp, TEAM = 1).  bvls_solve() answers what tg_batch_debug_bvls_solve answers on the device, EmuBvls.dynamics_inverse() /
EmuBvls.inverse_dynamics() what BatchMidpointVI.dynamics_inverse / inverse_dynamics answer with bounds=.  Test infrastructure only."""
import collections
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_LIB = None

DynamicsInverseBounded = collections.namedtuple("DynamicsInverseBounded", "U lam rho tau acc status rank active solves")
InverseDynamicsBounded = collections.namedtuple("InverseDynamicsBounded", "U lam P rho h status rank active solves")
BvlsAnswer = collections.namedtuple("BvlsAnswer", "z active solves rank status")


def sources():
    csrc = os.path.join(_ROOT, "trep_amd", "csrc")
    return [os.path.join(_HERE, "emu_bvls", "emu_bvls.cpp"), os.path.join(_ROOT, "include", "trep_amd.h")] + [
        os.path.join(csrc, f) for f in ("bvls_solve.hpp", "lsq_solve.hpp", "mvi_inverse_rows.hpp", "mvi_dyn_inverse.hpp", "mvi_inverse.hpp",
                                        "mvi_core.hpp", "lanes.hpp", "program.hpp", "devprog_fields.def", "schedule.hpp", "bbd.hpp",
                                        "bbd_solve.hpp", "dual.hpp", "gj_solve.hpp")]


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "emu_bvls", "libtrepamd_emu_bvls.so")
        srcs = sources()
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, srcs[0]], check=True)
        L = ctypes.CDLL(so)
        vp, i32, f64, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong
        L.emu_create.restype = vp
        L.emu_create.argtypes = [vp]
        L.emu_destroy.argtypes = [vp]
        L.emu_bvls_lds.argtypes = [vp, vp]
        L.emu_bvls_solve.argtypes = [i32, i32, i32, vp, vp, vp, vp, f64, i32, vp, vp, vp, vp, vp, i32]
        L.emu_dyn_inverse_bounded.argtypes = [vp, i32, i32, vp, i64, vp, i64, vp, i64, f64, f64, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                              vp, i32, i32, i32]
        L.emu_inverse_bounded.argtypes = [vp, i32, i32, f64, vp, vp, i64, vp, f64, f64, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32,
                                          i32, i32]
        _LIB = L
    return _LIB


def _ptr(x):
    return None if x is None or x.size == 0 else x.ctypes.data


def bvls_solve(A, c, lo, hi, rcond=1e-9, max_solves=0, poison=True):
    """A [count][rows][cols], c [count][rows], lo and hi [count][cols]: BvlsAnswer(z, active [count][cols], solves, rank, status [count])
    of the emulated solver."""
    A, c = np.ascontiguousarray(A, dtype=float), np.ascontiguousarray(c, dtype=float)
    count, rows, cols = A.shape
    lo = np.ascontiguousarray(np.broadcast_to(lo, (count, cols)), dtype=float)
    hi = np.ascontiguousarray(np.broadcast_to(hi, (count, cols)), dtype=float)
    z = np.full((count, cols), np.nan)
    active = np.full((count, cols), -9, dtype=np.int32)
    solves, rank, status = (np.full(count, -1, dtype=np.int32) for _ in range(3))
    lib().emu_bvls_solve(count, rows, cols, A.ctypes.data, c.ctypes.data, lo.ctypes.data, hi.ctypes.data, float(rcond), int(max_solves),
                         z.ctypes.data, active.ctypes.data, solves.ctypes.data, rank.ctypes.data, status.ctypes.data, 1 if poison else 0)
    return BvlsAnswer(z, active, solves, rank, status)


def box_rows(lo, hi, B, n):
    """(lo, hi, bound_rows) as contiguous [bound_rows][n] arrays from [n] or [B][n] boxes."""
    lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
    rows = B if (lo.ndim == 2 or hi.ndim == 2) else 1
    return (np.ascontiguousarray(np.broadcast_to(lo, (rows, n)), dtype=float), np.ascontiguousarray(np.broadcast_to(hi, (rows, n)), dtype=float), rows)


class EmuBvls(object):
    def __init__(self, desc):
        self.L = lib()
        self.h = self.L.emu_create(ctypes.addressof(desc.struct))
        assert self.h
        self.desc = desc
        self.nq, self.nd, self.nu, self.nc = int(desc.n_configs), int(desc.n_dyn), int(desc.n_inputs), int(desc.n_constraints)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.emu_destroy(self.h)
            self.h = None

    def lds_doubles(self):
        """Doubles of LDS per team: (computed torque BND, computed torque LSQ, inverse dynamics BND, inverse dynamics LSQ, rollout
        slice, o_kkt, o_ddq, o_scal of the first)."""
        out = np.zeros(8, dtype=np.int32)
        self.L.emu_bvls_lds(self.h, out.ctypes.data)
        return tuple(int(v) for v in out)

    def dynamics_inverse(self, Q, dQ, ddQ, lo, hi, ridge=0.0, rcond=1e-9, rows=None, group=1, strides=None, poison=True,
                         want=DynamicsInverseBounded._fields):
        Q, dQ, ddQ = (np.ascontiguousarray(a, dtype=float) for a in (Q, dQ, ddQ))
        B, M = Q.shape[0], Q.shape[1]
        n = self.nu + self.nc
        strides = tuple(a.shape[2] for a in (Q, dQ, ddQ)) if strides is None else strides
        rows = None if rows is None else np.ascontiguousarray(rows, dtype=float)
        lo, hi, bound_rows = box_rows(lo, hi, B, n)
        nan = lambda name, *shape: np.full(shape, np.nan) if name in want else None
        word = lambda name, *shape: np.full(shape, -9, dtype=np.int32) if name in want else None
        U, lam, rho = nan("U", B, M, self.nu), nan("lam", B, M, self.nc), nan("rho", B, M, self.nd)
        tau, acc = nan("tau", B, M, self.nd), nan("acc", B, M, self.nc)
        status, rank, active, solves = word("status", B, M), word("rank", B, M), word("active", B, M, n), word("solves", B, M)
        raw = lambda a: None if a is None else a.ctypes.data
        self.L.emu_dyn_inverse_bounded(self.h, B, M, Q.ctypes.data, int(strides[0]), dQ.ctypes.data, int(strides[1]), ddQ.ctypes.data,
                                       int(strides[2]), float(ridge), float(rcond), _ptr(lo), _ptr(hi), bound_rows, _ptr(U), _ptr(lam),
                                       _ptr(rho), _ptr(tau), _ptr(acc), raw(active), raw(solves), raw(rank), raw(status), _ptr(rows),
                                       int(group), 0 if rows is None else int(rows.shape[1]), 1 if poison else 0)
        return DynamicsInverseBounded(U, lam, rho, tau, acc, status, rank, active, solves)

    def inverse_dynamics(self, Q, dt, lo, hi, p0=None, ridge=0.0, rcond=1e-9, rows=None, group=1, stride=None, poison=True):
        Q = np.ascontiguousarray(Q, dtype=float)
        B, N = Q.shape[0], Q.shape[1] - 1
        n = self.nu + self.nc
        stride = Q.shape[2] if stride is None else stride
        dts = None if np.ndim(dt) == 0 else np.ascontiguousarray(dt, dtype=float)
        p0 = None if p0 is None else np.ascontiguousarray(p0, dtype=float)
        rows = None if rows is None else np.ascontiguousarray(rows, dtype=float)
        lo, hi, bound_rows = box_rows(lo, hi, B, n)
        nan = lambda *shape: np.full(shape, np.nan)
        U, lam, P, rho, h = nan(B, N, self.nu), nan(B, N, self.nc), nan(B, N + 1, self.nd), nan(B, N, self.nd), nan(B, N, self.nc)
        status, rank, solves = (np.full((B, N), -9, dtype=np.int32) for _ in range(3))
        active = np.full((B, N, n), -9, dtype=np.int32)
        self.L.emu_inverse_bounded(self.h, B, N, float(dt) if dts is None else float(dts[0]), _ptr(dts), Q.ctypes.data, int(stride), _ptr(p0),
                                   float(ridge), float(rcond), _ptr(lo), _ptr(hi), bound_rows, _ptr(U), _ptr(lam), _ptr(P), _ptr(rho), _ptr(h),
                                   active.ctypes.data, solves.ctypes.data, rank.ctypes.data, status.ctypes.data, _ptr(rows), int(group),
                                   0 if rows is None else int(rows.shape[1]), 1 if poison else 0)
        return InverseDynamicsBounded(U, lam, P, rho, h, status, rank, active, solves)
