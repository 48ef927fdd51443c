"""ctypes driver for the host emulation of the tape-measure kernel (tests/emu_tape/emu_tape.cpp, compiled on demand with g++ from
trep_amd/csrc/mvi_tape.hpp, TEAM = 1).  EmuTape.tape_measures() answers what BatchMidpointVI.tape_measures answers on the device,
with NaN-poisoned outputs.  Test infrastructure only."""
import collections
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_LIB = None

FIELDS = ("length", "velocity", "length_dq", "velocity_dq", "length_dqdq")
TapeMeasures = collections.namedtuple("TapeMeasures", FIELDS)


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "emu_tape", "libtrepamd_emu_tape.so")
        csrc = os.path.join(_ROOT, "trep_amd", "csrc")
        srcs = [os.path.join(_HERE, "emu_tape", "emu_tape.cpp"), os.path.join(_ROOT, "include", "trep_amd.h")] + [
            os.path.join(csrc, f) for f in ("mvi_tape.hpp", "mvi_frames.hpp", "mvi_core.hpp", "lanes.hpp", "program.hpp", "devprog_fields.def",
                                            "schedule.hpp", "bbd.hpp", "bbd_solve.hpp", "dual.hpp", "gj_solve.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, srcs[0]], check=True)
        L = ctypes.CDLL(so)
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
        L.emu_create.restype = vp
        L.emu_create.argtypes = [vp]
        L.emu_destroy.argtypes = [vp]
        L.emu_tape_lds.argtypes = [vp, i32, vp]
        L.emu_tape_table.argtypes = [vp, i32, vp, vp, vp, vp]
        L.emu_tape.restype = i32
        L.emu_tape.argtypes = [vp, i32, i32, vp, i64, vp, i64, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32]
        _LIB = L
    return _LIB


def flatten(measures):
    """Lists of frame indices -> (start [T + 1], frames) as int32, the layout of tg_batch_tape_measures."""
    start = np.zeros(len(measures) + 1, dtype=np.int32)
    start[1:] = np.cumsum([len(m) for m in measures])
    return start, np.array([f for m in measures for f in m], dtype=np.int32)


class EmuTape(object):
    def __init__(self, desc):
        self.L = lib()
        self.h = self.L.emu_create(ctypes.addressof(desc.struct))
        assert self.h
        self.desc = desc
        self.nq, self.n_frames = int(desc.n_configs), int(desc.n_frames)
        self.built = None

    def __del__(self):
        if getattr(self, "h", None):
            self.L.emu_destroy(self.h)
            self.h = None

    def lds_doubles(self, longest):
        """(doubles of LDS per team of the kernel for a longest measure of `longest` segments, of the rollout slice)."""
        out = np.zeros(3, dtype=np.int32)
        self.L.emu_tape_lds(self.h, int(longest), out.ctypes.data)
        assert out[2] == self.n_frames
        return int(out[0]), int(out[1])

    def table(self, measures):
        """dict(unique=, segments=, longest=, cuts=[measure index where every pass begins ..., T]) of a selection."""
        start, frames = flatten(measures)
        out, cuts = np.zeros(4, dtype=np.int32), np.zeros(len(measures) + 1, dtype=np.int32)
        self.L.emu_tape_table(self.h, len(measures), start.ctypes.data, frames.ctypes.data, out.ctypes.data, cuts.ctypes.data)
        return dict(unique=int(out[0]), segments=int(out[1]), longest=int(out[3]), cuts=[int(c) for c in cuts[:out[2] + 1]])

    def tape_measures(self, Q, dQ=None, measures=None, gradients=True, hessians=True, want_length=True, q_stride=None, reuse=False, poison=True):
        """Q [B][M][>= nq] (q_stride: doubles per row, default its last dimension), dQ likewise or None; measures: lists of frame
        indices.  Outputs start as NaN: whatever the kernel leaves unwritten shows.  self.built: was the table built by this call."""
        Q = np.ascontiguousarray(Q, dtype=float)
        B, M = Q.shape[0], Q.shape[1]
        dQ = None if dQ is None else np.ascontiguousarray(dQ, dtype=float)
        for m in measures:
            assert len(m) >= 2 and min(m) >= 0 and max(m) < self.n_frames and all(a != b for a, b in zip(m[:-1], m[1:]))
        start, frames = flatten(measures)
        T, nq = len(measures), self.nq
        nan = lambda *shape: np.full(shape, np.nan)
        length = nan(B, M, T) if want_length else None
        velocity = None if dQ is None else nan(B, M, T)
        length_dq = nan(B, M, T, nq) if gradients else None
        velocity_dq = nan(B, M, T, nq) if gradients and dQ is not None else None
        length_dqdq = nan(B, M, T, nq, nq) if hessians else None
        ptr = lambda a: None if a is None else a.ctypes.data
        self.built = bool(self.L.emu_tape(self.h, B, M, Q.ctypes.data, int(Q.shape[2] if q_stride is None else q_stride), ptr(dQ),
                                          0 if dQ is None else int(dQ.shape[2]), T, start.ctypes.data, frames.ctypes.data, ptr(length),
                                          ptr(velocity), ptr(length_dq), ptr(velocity_dq), ptr(length_dqdq), 1 if reuse else 0, 1 if poison else 0))
        return TapeMeasures(length, velocity, length_dq, velocity_dq, length_dqdq)
