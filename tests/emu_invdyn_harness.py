"""ctypes driver for the host emulation of the inverse-dynamics kernel (tests/emu_invdyn/emu_invdyn.cpp, compiled on demand with g++
from trep_amd/csrc/mvi_inverse.hpp, TEAM = 1).  EmuInverse.inverse_dynamics() answers what BatchMidpointVI.inverse_dynamics answers on
the device.  Test infrastructure only."""
import collections
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_LIB = None

InverseDynamics = collections.namedtuple("InverseDynamics", "U lam P rho h status")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "emu_invdyn", "libtrepamd_emu_invdyn.so")
        csrc = os.path.join(_ROOT, "trep_amd", "csrc")
        srcs = [os.path.join(_HERE, "emu_invdyn", "emu_invdyn.cpp"), os.path.join(_ROOT, "include", "trep_amd.h")] + [
            os.path.join(csrc, f) for f in ("mvi_inverse.hpp", "mvi_core.hpp", "lanes.hpp", "program.hpp", "devprog_fields.def",
                                            "schedule.hpp", "bbd.hpp", "bbd_solve.hpp", "dual.hpp", "gj_solve.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, srcs[0]], check=True)
        L = ctypes.CDLL(so)
        vp, i32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        L.emu_create.restype = vp
        L.emu_create.argtypes = [vp]
        L.emu_destroy.argtypes = [vp]
        L.emu_inverse_lds.argtypes = [vp, vp]
        L.emu_inverse.argtypes = [vp, i32, i32, f64, vp, vp, ctypes.c_longlong, vp, f64, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32]
        _LIB = L
    return _LIB


def _ptr(x):
    return None if x is None or x.size == 0 else x.ctypes.data


class EmuInverse(object):
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
        """(doubles of LDS per team of the kernel, of the rollout slice)."""
        out = np.zeros(2, dtype=np.int32)
        self.L.emu_inverse_lds(self.h, out.ctypes.data)
        return int(out[0]), int(out[1])

    def inverse_dynamics(self, Q, dt, p0=None, ridge=0.0, rows=None, group=1, stride=None, poison=True):
        """Q [B][N+1][>= nq] (stride: doubles per row, default its last dimension); dt a scalar or [N]; rows [R][width]: a parameter
        table (mass, Ixx, Iyy, Izz of every body | gravity [3] | damping [nd]), trajectory b using row b // group."""
        Q = np.ascontiguousarray(Q, dtype=float)
        B, N = Q.shape[0], Q.shape[1] - 1
        stride = Q.shape[2] if stride is None else stride
        dts = None if np.ndim(dt) == 0 else np.ascontiguousarray(dt, dtype=float)
        p0 = None if p0 is None else np.ascontiguousarray(p0, dtype=float)
        rows = None if rows is None else np.ascontiguousarray(rows, dtype=float)
        nan = lambda *shape: np.full(shape, np.nan)
        U, lam, P, rho, h = nan(B, N, self.nu), nan(B, N, self.nc), nan(B, N + 1, self.nd), nan(B, N, self.nd), nan(B, N, self.nc)
        status = np.full((B, N), -1, dtype=np.int32)
        self.L.emu_inverse(self.h, B, N, float(dt) if dts is None else float(dts[0]), _ptr(dts), Q.ctypes.data, int(stride), _ptr(p0),
                           float(ridge), _ptr(U), _ptr(lam), _ptr(P), _ptr(rho), _ptr(h), status.ctypes.data, _ptr(rows), int(group),
                           0 if rows is None else int(rows.shape[1]), 1 if poison else 0)
        return InverseDynamics(U, lam, P, rho, h, status)
