"""ctypes driver for the host emulation of the rank-revealing least-squares solver and of the two kernels that end in it
(tests/emu_lsq/emu_lsq.cpp, compiled on demand with g++ from trep_amd/csrc/lsq_solve.hpp, mvi_dyn_inverse.hpp and mvi_inverse.hpp,
TEAM = 1).  lsq_solve() answers what tg_batch_debug_lsq_solve answers on the device, EmuLsq.dynamics_inverse() /
EmuLsq.inverse_dynamics() what BatchMidpointVI.dynamics_inverse / inverse_dynamics answer with rcond=.  Test infrastructure only."""
import collections
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_LIB = None

DynamicsInverseRank = collections.namedtuple("DynamicsInverseRank", "U lam rho tau acc status rank")
InverseDynamicsRank = collections.namedtuple("InverseDynamicsRank", "U lam P rho h status rank")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "emu_lsq", "libtrepamd_emu_lsq.so")
        csrc = os.path.join(_ROOT, "trep_amd", "csrc")
        srcs = [os.path.join(_HERE, "emu_lsq", "emu_lsq.cpp"), os.path.join(_ROOT, "include", "trep_amd.h")] + [
            os.path.join(csrc, f) for f in ("lsq_solve.hpp", "mvi_inverse_rows.hpp", "mvi_dyn_inverse.hpp", "mvi_inverse.hpp", "mvi_core.hpp",
                                            "lanes.hpp", "program.hpp", "devprog_fields.def", "schedule.hpp", "bbd.hpp", "bbd_solve.hpp",
                                            "dual.hpp", "gj_solve.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, srcs[0]], check=True)
        L = ctypes.CDLL(so)
        vp, i32, f64, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong
        L.emu_create.restype = vp
        L.emu_create.argtypes = [vp]
        L.emu_destroy.argtypes = [vp]
        L.emu_lsq_lds.argtypes = [vp, vp]
        L.emu_lsq_solve.argtypes = [i32, i32, i32, vp, vp, f64, vp, vp, vp, i32]
        L.emu_dyn_inverse_lsq.argtypes = [vp, i32, i32, vp, i64, vp, i64, vp, i64, f64, f64, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32]
        L.emu_inverse_lsq.argtypes = [vp, i32, i32, f64, vp, vp, i64, vp, f64, f64, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32]
        _LIB = L
    return _LIB


def _ptr(x):
    return None if x is None or x.size == 0 else x.ctypes.data


def lsq_solve(A, c, rcond, poison=True):
    """A [count][rows][cols], c [count][rows]: (z [count][cols], rank [count], status [count]) of the emulated solver."""
    A, c = np.ascontiguousarray(A, dtype=float), np.ascontiguousarray(c, dtype=float)
    count, rows, cols = A.shape
    z = np.full((count, cols), np.nan)
    rank, status = np.full(count, -1, dtype=np.int32), np.full(count, -1, dtype=np.int32)
    lib().emu_lsq_solve(count, rows, cols, A.ctypes.data, c.ctypes.data, float(rcond), z.ctypes.data, rank.ctypes.data, status.ctypes.data,
                        1 if poison else 0)
    return z, rank, status


class EmuLsq(object):
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
        """Doubles of LDS per team: (computed torque LSQ, computed torque, inverse dynamics LSQ, inverse dynamics, rollout slice,
        o_kkt, o_ddq, o_scal of the first)."""
        out = np.zeros(8, dtype=np.int32)
        self.L.emu_lsq_lds(self.h, out.ctypes.data)
        return tuple(int(v) for v in out)

    def dynamics_inverse(self, Q, dQ, ddQ, ridge=0.0, rcond=1e-9, rows=None, group=1, strides=None, poison=True, want=DynamicsInverseRank._fields):
        """As EmuDynInverse.dynamics_inverse (emu_dyn_inverse_harness.py), through the LSQ instantiation: rank is one more output."""
        Q, dQ, ddQ = (np.ascontiguousarray(a, dtype=float) for a in (Q, dQ, ddQ))
        B, M = Q.shape[0], Q.shape[1]
        strides = tuple(a.shape[2] for a in (Q, dQ, ddQ)) if strides is None else strides
        rows = None if rows is None else np.ascontiguousarray(rows, dtype=float)
        nan = lambda name, *shape: np.full(shape, np.nan) if name in want else None
        U, lam, rho = nan("U", B, M, self.nu), nan("lam", B, M, self.nc), nan("rho", B, M, self.nd)
        tau, acc = nan("tau", B, M, self.nd), nan("acc", B, M, self.nc)
        status = np.full((B, M), -1, dtype=np.int32) if "status" in want else None
        rank = np.full((B, M), -1, dtype=np.int32) if "rank" in want else None
        self.L.emu_dyn_inverse_lsq(self.h, B, M, Q.ctypes.data, int(strides[0]), dQ.ctypes.data, int(strides[1]), ddQ.ctypes.data,
                                   int(strides[2]), float(ridge), float(rcond), _ptr(U), _ptr(lam), _ptr(rho), _ptr(tau), _ptr(acc),
                                   None if rank is None else rank.ctypes.data, None if status is None else status.ctypes.data,
                                   _ptr(rows), int(group), 0 if rows is None else int(rows.shape[1]), 1 if poison else 0)
        return DynamicsInverseRank(U, lam, rho, tau, acc, status, rank)

    def inverse_dynamics(self, Q, dt, p0=None, ridge=0.0, rcond=1e-9, rows=None, group=1, stride=None, poison=True):
        """As EmuInverse.inverse_dynamics (emu_invdyn_harness.py), through the LSQ instantiation: rank is one more output."""
        Q = np.ascontiguousarray(Q, dtype=float)
        B, N = Q.shape[0], Q.shape[1] - 1
        stride = Q.shape[2] if stride is None else stride
        dts = None if np.ndim(dt) == 0 else np.ascontiguousarray(dt, dtype=float)
        p0 = None if p0 is None else np.ascontiguousarray(p0, dtype=float)
        rows = None if rows is None else np.ascontiguousarray(rows, dtype=float)
        nan = lambda *shape: np.full(shape, np.nan)
        U, lam, P, rho, h = nan(B, N, self.nu), nan(B, N, self.nc), nan(B, N + 1, self.nd), nan(B, N, self.nd), nan(B, N, self.nc)
        status, rank = np.full((B, N), -1, dtype=np.int32), np.full((B, N), -1, dtype=np.int32)
        self.L.emu_inverse_lsq(self.h, B, N, float(dt) if dts is None else float(dts[0]), _ptr(dts), Q.ctypes.data, int(stride), _ptr(p0),
                               float(ridge), float(rcond), _ptr(U), _ptr(lam), _ptr(P), _ptr(rho), _ptr(h), rank.ctypes.data,
                               status.ctypes.data, _ptr(rows), int(group), 0 if rows is None else int(rows.shape[1]), 1 if poison else 0)
        return InverseDynamicsRank(U, lam, P, rho, h, status, rank)
