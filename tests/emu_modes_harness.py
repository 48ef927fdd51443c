"""ctypes driver for the host emulation of the normal-modes kernel (tests/emu_modes/emu_modes.cpp, compiled on demand with g++ from
trep_amd/csrc/mvi_modes.hpp, TEAM = 1).  EmuModes.normal_modes() answers what BatchMidpointVI.normal_modes answers on the device.
Test infrastructure only."""
import collections
import ctypes
import os
import subprocess

import numpy as np

import emu_harness

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_LIB = None

NormalModes = collections.namedtuple("NormalModes", "omega2 modes count rank mu residual sweeps status")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "emu_modes", "libtrepamd_emu_modes.so")
        csrc = os.path.join(_ROOT, "trep_amd", "csrc")
        srcs = [os.path.join(_HERE, "emu_modes", "emu_modes.cpp"), os.path.join(_ROOT, "include", "trep_amd.h")] + [
            os.path.join(csrc, f) for f in ("mvi_pose.hpp", "mvi_modes.hpp", "sym_eig.hpp", "lsq_solve.hpp", "mvi_core.hpp", "lanes.hpp",
                                            "program.hpp", "devprog_fields.def", "schedule.hpp", "bbd.hpp", "bbd_solve.hpp", "dual.hpp",
                                            "gj_solve.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, srcs[0]], check=True)
        L = ctypes.CDLL(so)
        L.emu_create.restype = ctypes.c_void_p
        L.emu_create.argtypes = [ctypes.c_void_p]
        L.emu_destroy.argtypes = [ctypes.c_void_p]
        L.emu_sizeof_run_args.restype = ctypes.c_int
        L.emu_modes_lds.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.emu_modes.argtypes = ([ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_double, ctypes.c_int] +
                                [ctypes.c_void_p] * 7 + [ctypes.c_int, ctypes.c_int])
        _LIB = L
    return _LIB


def _ptr(x):
    return None if x is None or x.size == 0 else x.ctypes.data


class EmuModes(object):
    MODE = 15

    def __init__(self, desc):
        self.L = lib()
        assert int(self.L.emu_sizeof_run_args()) == ctypes.sizeof(emu_harness.RunArgs)
        self.h = self.L.emu_create(ctypes.addressof(desc.struct))
        assert self.h
        self.desc = desc
        self.nq, self.nd, self.nc = int(desc.n_configs), int(desc.n_dyn), int(desc.n_constraints)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.emu_destroy(self.h)
            self.h = None

    def lds_doubles(self):
        """(doubles of LDS per team of the kernel, of the rollout slice)."""
        out = np.zeros(2, dtype=np.int32)
        self.L.emu_modes_lds(self.h, out.ctypes.data)
        return int(out[0]), int(out[1])

    def normal_modes(self, Q, mu=None, free=None, rcond=1e-9, max_sweeps=30, rows=None, group=1):
        """free: boolean / int mask [nq] or None (every dynamic config; a kinematic config is cleared, as the library's host does).
        rows [R][stride]: a parameter table, pose t using row t // group."""
        Q = np.ascontiguousarray(Q, dtype=float)
        B = Q.shape[0]
        assert Q.shape == (B, self.nq)
        mask = np.zeros(self.nq, dtype=np.int32)
        mask[:self.nd] = 1 if free is None else (np.asarray(free)[:self.nd] != 0)
        nF = int(mask.sum())
        mu_in = None if mu is None else np.ascontiguousarray(mu, dtype=float).reshape(B, self.nc)
        rows = None if rows is None else np.ascontiguousarray(rows, dtype=float)
        omega2, modes = np.full((B, nF), np.nan), np.full((B, nF, self.nq), np.nan)
        count, rank = np.full(B, -1, dtype=np.int32), np.full(B, -1, dtype=np.int32)
        mu_out, residual = np.full((B, self.nc), np.nan), np.full(B, np.nan)
        sweeps, status = np.full(B, -1, dtype=np.int32), np.full(B, -1, dtype=np.int32)
        a = emu_harness.RunArgs()
        a.batch, a.mode, a.max_iterations, a.tolerance = B, self.MODE, int(max_sweeps), 1.0
        a.group_size = 1
        a.iters = sweeps.ctypes.data_as(emu_harness._I)
        a.status = status.ctypes.data_as(emu_harness._I)
        self.L.emu_modes(self.h, ctypes.addressof(a), mask.ctypes.data, nF, _ptr(Q), _ptr(mu_in), float(rcond), int(max_sweeps), _ptr(omega2),
                         _ptr(modes), count.ctypes.data, rank.ctypes.data, _ptr(mu_out), residual.ctypes.data, _ptr(rows), int(group),
                         0 if rows is None else int(rows.shape[1]))
        return NormalModes(omega2, modes, count, rank, mu_out, residual, sweeps, status)
