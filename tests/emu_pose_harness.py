"""ctypes driver for the host emulation of the pose-solver kernels (tests/emu_pose/emu_pose.cpp, compiled on demand with g++ from
trep_amd/csrc/mvi_project.hpp and mvi_equilibrium.hpp, TEAM = 1).  EmuProjection.project() answers what
BatchMidpointVI.satisfy_constraints answers on the device, EmuEquilibrium.minimize() what minimize_potential_energy does.  Test
infrastructure only."""
import collections
import ctypes
import os
import subprocess

import numpy as np

import emu_harness

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_LIB = None

Projection = collections.namedtuple("Projection", "Q dQ mu iterations status")
Equilibrium = collections.namedtuple("Equilibrium", "Q mu V iterations status")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "emu_pose", "libtrepamd_emu_pose.so")
        csrc = os.path.join(_ROOT, "trep_amd", "csrc")
        srcs = [os.path.join(_HERE, "emu_pose", "emu_pose.cpp"), os.path.join(_ROOT, "include", "trep_amd.h")] + [
            os.path.join(csrc, f) for f in ("mvi_pose.hpp", "mvi_project.hpp", "mvi_equilibrium.hpp", "mvi_core.hpp", "lanes.hpp",
                                            "program.hpp", "devprog_fields.def", "schedule.hpp", "bbd.hpp", "bbd_solve.hpp", "dual.hpp",
                                            "gj_solve.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, srcs[0]], check=True)
        L = ctypes.CDLL(so)
        L.emu_create.restype = ctypes.c_void_p
        L.emu_create.argtypes = [ctypes.c_void_p]
        L.emu_destroy.argtypes = [ctypes.c_void_p]
        L.emu_sizeof_run_args.restype = ctypes.c_int
        L.emu_project_lds.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.emu_project.argtypes = [ctypes.c_void_p] * 8
        L.emu_equilibrium_lds.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.emu_equilibrium.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        _LIB = L
    return _LIB


def sizeof_run_args():
    """sizeof(tg::RunArgs) in the kernels' own translation unit."""
    return int(lib().emu_sizeof_run_args())


def _ptr(x):
    return None if x is None or x.size == 0 else x.ctypes.data


class EmuPose(object):
    """One system in the emulation; the subclasses name their kernel's mode and geometry call."""
    MODE = None
    LDS = None

    def __init__(self, desc):
        self.L = lib()
        self.h = self.L.emu_create(ctypes.addressof(desc.struct))
        assert self.h
        self.desc = desc
        self.nq, self.nc = int(desc.n_configs), int(desc.n_constraints)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.emu_destroy(self.h)
            self.h = None

    def lds_doubles(self):
        """(doubles of LDS per team of the kernel, of the rollout slice)."""
        out = np.zeros(2, dtype=np.int32)
        getattr(self.L, self.LDS)(self.h, out.ctypes.data)
        return int(out[0]), int(out[1])

    def _call(self, Q, free, tolerance, max_iterations):
        """The checked inputs, the outputs every solver has and the filled RunArgs: (Q, mask, q, mu, iters, status, args)."""
        Q = np.ascontiguousarray(Q, dtype=float)
        B = Q.shape[0]
        assert Q.shape == (B, self.nq)
        mask = None if free is None else np.ascontiguousarray(np.asarray(free) != 0, dtype=np.int32)
        q, mu = np.zeros((B, self.nq)), np.zeros((B, self.nc))
        iters, status = np.full(B, -1, dtype=np.int32), np.full(B, -1, dtype=np.int32)
        a = emu_harness.RunArgs()
        a.batch, a.mode, a.max_iterations, a.tolerance = B, self.MODE, int(max_iterations), float(tolerance)
        a.group_size = 1
        a.iters = iters.ctypes.data_as(emu_harness._I)
        a.status = status.ctypes.data_as(emu_harness._I)
        return Q, mask, q, mu, iters, status, a


class EmuProjection(EmuPose):
    MODE, LDS = 9, "emu_project_lds"

    def project(self, Q, dQ=None, free=None, tolerance=1e-10, max_iterations=50):
        """free: boolean / int mask [nq] or None (every config)."""
        Q, mask, q, mu, iters, status, a = self._call(Q, free, tolerance, max_iterations)
        dQ = None if dQ is None else np.ascontiguousarray(dQ, dtype=float)
        dq = None if dQ is None else np.zeros(Q.shape)
        self.L.emu_project(self.h, ctypes.addressof(a), _ptr(mask), _ptr(Q), _ptr(dQ), _ptr(q), _ptr(dq), _ptr(mu))
        return Projection(q, dq, mu, iters, status)


class EmuEquilibrium(EmuPose):
    MODE, LDS = 10, "emu_equilibrium_lds"

    def minimize(self, Q, free=None, tolerance=1e-10, max_iterations=100, rows=None, group=1):
        """free: boolean / int mask [nq] or None (every config).  rows [R][stride]: a parameter table (mass, Ixx, Iyy, Izz of every
        body | gravity [3] | damping [nd]), pose t using row t // group."""
        Q, mask, q, mu, iters, status, a = self._call(Q, free, tolerance, max_iterations)
        rows = None if rows is None else np.ascontiguousarray(rows, dtype=float)
        v = np.zeros((Q.shape[0], 2))
        self.L.emu_equilibrium(self.h, ctypes.addressof(a), _ptr(mask), _ptr(Q), _ptr(q), _ptr(mu), _ptr(v), _ptr(rows), int(group),
                               0 if rows is None else int(rows.shape[1]))
        return Equilibrium(q, mu, v, iters, status)
