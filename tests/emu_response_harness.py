"""ctypes driver for the host emulation of the static-response kernel (tests/emu_response/emu_response.cpp, compiled on demand with
g++ from trep_amd/csrc/mvi_response.hpp, TEAM = 1).  EmuResponse.static_response() answers what BatchMidpointVI.static_response
answers on the device.  Test infrastructure only."""
import collections
import ctypes
import os
import subprocess

import numpy as np

import emu_harness

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_LIB = None

StaticResponse = collections.namedtuple("StaticResponse", "dq dmu compliance reaction rank mu residual defect status")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "emu_response", "libtrepamd_emu_response.so")
        csrc = os.path.join(_ROOT, "trep_amd", "csrc")
        srcs = [os.path.join(_HERE, "emu_response", "emu_response.cpp"), os.path.join(_ROOT, "include", "trep_amd.h")] + [
            os.path.join(csrc, f) for f in ("mvi_pose.hpp", "mvi_response.hpp", "lsq_solve.hpp", "mvi_core.hpp", "lanes.hpp", "program.hpp",
                                            "devprog_fields.def", "schedule.hpp", "bbd.hpp", "bbd_solve.hpp", "dual.hpp", "gj_solve.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, srcs[0]], check=True)
        L = ctypes.CDLL(so)
        L.emu_create.restype = ctypes.c_void_p
        L.emu_create.argtypes = [ctypes.c_void_p]
        L.emu_destroy.argtypes = [ctypes.c_void_p]
        L.emu_sizeof_run_args.restype = ctypes.c_int
        L.emu_response_lds.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        L.emu_response.argtypes = ([ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_double, ctypes.c_int] +
                                   [ctypes.c_void_p] * 9 + [ctypes.c_int, ctypes.c_int])
        _LIB = L
    return _LIB


def _ptr(x):
    return None if x is None or x.size == 0 else x.ctypes.data


class EmuResponse(object):
    MODE = 16

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

    def lds_doubles(self, n_free, n_drive, compliance=True):
        """(doubles of LDS per team of the kernel, of the rollout slice)."""
        out = np.zeros(2, dtype=np.int32)
        self.L.emu_response_lds(self.h, int(n_free), int(n_drive), int(bool(compliance)), out.ctypes.data)
        return int(out[0]), int(out[1])

    def static_response(self, Q, free, mu=None, drive=None, compliance=True, rcond=1e-9, rows=None, group=1):
        """free: boolean / int mask [nq]; drive: config indices among the held ones (None: all of them, in config order).
        rows [R][stride]: a parameter table, pose t using row t // group."""
        Q = np.ascontiguousarray(Q, dtype=float)
        B = Q.shape[0]
        assert Q.shape == (B, self.nq)
        mask = np.ascontiguousarray(np.asarray(free) != 0, dtype=np.int32)
        nF = int(mask.sum())
        drive = np.flatnonzero(mask == 0) if drive is None else np.asarray(drive)
        drive = np.ascontiguousarray(drive, dtype=np.int32)
        assert not mask[drive].any() and len(set(drive.tolist())) == len(drive)
        nD = len(drive)
        mu_in = None if mu is None else np.ascontiguousarray(mu, dtype=float).reshape(B, self.nc)
        rows = None if rows is None else np.ascontiguousarray(rows, dtype=float)
        dq, dmu = np.full((B, nD, self.nq), np.nan), np.full((B, nD, self.nc), np.nan)
        C = np.full((B, self.nq, self.nq), np.nan) if compliance else None
        R = np.full((B, self.nq, self.nc), np.nan) if compliance else None
        rank = np.full(B, -1, dtype=np.int32)
        mu_out, residual, defect = np.full((B, self.nc), np.nan), np.full(B, np.nan), np.full(B, np.nan)
        iters, status = np.full(B, -1, dtype=np.int32), np.full(B, -1, dtype=np.int32)
        a = emu_harness.RunArgs()
        a.batch, a.mode, a.max_iterations, a.tolerance = B, self.MODE, 0, 1.0
        a.group_size = 1
        a.iters = iters.ctypes.data_as(emu_harness._I)
        a.status = status.ctypes.data_as(emu_harness._I)
        self.L.emu_response(self.h, ctypes.addressof(a), mask.ctypes.data, nF, _ptr(drive), nD, _ptr(Q), _ptr(mu_in), float(rcond), int(bool(compliance)), _ptr(dq),
                            _ptr(dmu), _ptr(C), _ptr(R), rank.ctypes.data, _ptr(mu_out), residual.ctypes.data,
                            defect.ctypes.data, _ptr(rows), int(group), 0 if rows is None else int(rows.shape[1]))
        return StaticResponse(dq, dmu, C, R, rank, mu_out, residual, defect, status)
