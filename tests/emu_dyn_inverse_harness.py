"""ctypes driver for the host emulation of the computed-torque kernel (tests/emu_dyn_inverse/emu_dyn_inverse.cpp, compiled on demand with
g++ from trep_amd/csrc/mvi_dyn_inverse.hpp, TEAM = 1).  EmuDynInverse.dynamics_inverse() answers what BatchMidpointVI.dynamics_inverse
answers on the device.  Test infrastructure only."""
import collections
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_LIB = None

DynamicsInverse = collections.namedtuple("DynamicsInverse", "U lam rho tau acc status")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "emu_dyn_inverse", "libtrepamd_emu_dyn_inverse.so")
        csrc = os.path.join(_ROOT, "trep_amd", "csrc")
        srcs = [os.path.join(_HERE, "emu_dyn_inverse", "emu_dyn_inverse.cpp"), os.path.join(_ROOT, "include", "trep_amd.h")] + [
            os.path.join(csrc, f) for f in ("mvi_dyn_inverse.hpp", "mvi_core.hpp", "lanes.hpp", "program.hpp", "devprog_fields.def",
                                            "schedule.hpp", "bbd.hpp", "bbd_solve.hpp", "dual.hpp", "gj_solve.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, srcs[0]], check=True)
        L = ctypes.CDLL(so)
        vp, i32, f64, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong
        L.emu_create.restype = vp
        L.emu_create.argtypes = [vp]
        L.emu_destroy.argtypes = [vp]
        L.emu_dyn_inverse_lds.argtypes = [vp, vp]
        L.emu_dyn_inverse.argtypes = [vp, i32, i32, vp, i64, vp, i64, vp, i64, f64, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32]
        _LIB = L
    return _LIB


def _ptr(x):
    return None if x is None or x.size == 0 else x.ctypes.data


class EmuDynInverse(object):
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
        """(doubles of LDS per team of the kernel, of the rollout slice, the offsets of the image, the accelerations and the row scales)."""
        out = np.zeros(5, dtype=np.int32)
        self.L.emu_dyn_inverse_lds(self.h, out.ctypes.data)
        return tuple(int(v) for v in out)

    def dynamics_inverse(self, Q, dQ, ddQ, ridge=0.0, rows=None, group=1, strides=None, poison=True, want=DynamicsInverse._fields):
        """Q, dQ, ddQ [B][M][>= nq] (strides: doubles per row of each, default their last dimensions); rows [R][width]: a parameter
        table (mass, Ixx, Iyy, Izz of every body | gravity [3] | damping [nd]), trajectory b using row b // group; want: the outputs
        asked for (the others are passed as null and come back None)."""
        Q, dQ, ddQ = (np.ascontiguousarray(a, dtype=float) for a in (Q, dQ, ddQ))
        B, M = Q.shape[0], Q.shape[1]
        strides = tuple(a.shape[2] for a in (Q, dQ, ddQ)) if strides is None else strides
        rows = None if rows is None else np.ascontiguousarray(rows, dtype=float)
        nan = lambda name, *shape: np.full(shape, np.nan) if name in want else None
        U, lam, rho = nan("U", B, M, self.nu), nan("lam", B, M, self.nc), nan("rho", B, M, self.nd)
        tau, acc = nan("tau", B, M, self.nd), nan("acc", B, M, self.nc)
        status = np.full((B, M), -1, dtype=np.int32) if "status" in want else None
        self.L.emu_dyn_inverse(self.h, B, M, Q.ctypes.data, int(strides[0]), dQ.ctypes.data, int(strides[1]), ddQ.ctypes.data, int(strides[2]),
                               float(ridge), _ptr(U), _ptr(lam), _ptr(rho), _ptr(tau), _ptr(acc), None if status is None else status.ctypes.data,
                               _ptr(rows), int(group), 0 if rows is None else int(rows.shape[1]), 1 if poison else 0)
        return DynamicsInverse(U, lam, rho, tau, acc, status)
