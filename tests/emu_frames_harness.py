"""ctypes driver for the host emulation of the frame-kinematics kernel (tests/emu_frames/emu_frames.cpp, compiled on demand with g++
from trep_amd/csrc/mvi_frames.hpp, TEAM = 1).  EmuFrames.frame_kinematics() answers what BatchMidpointVI.frame_kinematics answers on
the device, with NaN-poisoned outputs.  Test infrastructure only."""
import collections
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_LIB = None

FrameKinematics = collections.namedtuple("FrameKinematics", "g vb p_dq vb_ddq")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "emu_frames", "libtrepamd_emu_frames.so")
        csrc = os.path.join(_ROOT, "trep_amd", "csrc")
        srcs = [os.path.join(_HERE, "emu_frames", "emu_frames.cpp"), os.path.join(_ROOT, "include", "trep_amd.h")] + [
            os.path.join(csrc, f) for f in ("mvi_frames.hpp", "mvi_core.hpp", "lanes.hpp", "program.hpp", "devprog_fields.def",
                                            "schedule.hpp", "bbd.hpp", "bbd_solve.hpp", "dual.hpp", "gj_solve.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, srcs[0]], check=True)
        L = ctypes.CDLL(so)
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
        L.emu_create.restype = vp
        L.emu_create.argtypes = [vp]
        L.emu_destroy.argtypes = [vp]
        L.emu_frames_lds.argtypes = [vp, vp]
        L.emu_frame_anchors.argtypes = [vp, vp]
        L.emu_frames.argtypes = [vp, i32, i32, vp, i64, vp, i64, i32, vp, vp, vp, vp, vp, i32]
        _LIB = L
    return _LIB


class EmuFrames(object):
    def __init__(self, desc):
        self.L = lib()
        self.h = self.L.emu_create(ctypes.addressof(desc.struct))
        assert self.h
        self.desc = desc
        self.nq, self.n_frames = int(desc.n_configs), int(desc.n_frames)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.emu_destroy(self.h)
            self.h = None

    def lds_doubles(self):
        """(doubles of LDS per team of the kernel, of the rollout slice)."""
        out = np.zeros(3, dtype=np.int32)
        self.L.emu_frames_lds(self.h, out.ctypes.data)
        assert out[2] == self.n_frames
        return int(out[0]), int(out[1])

    def anchors(self):
        """The anchor joint of every frame (-1: no variable ancestor)."""
        out = np.zeros(self.n_frames, dtype=np.int32)
        self.L.emu_frame_anchors(self.h, out.ctypes.data)
        return out

    def frame_kinematics(self, Q, dQ=None, frames=None, jacobians=True, want_g=True, q_stride=None, poison=True):
        """Q [B][M][>= nq] (q_stride: doubles per row, default its last dimension), dQ likewise or None; frames: indices (default
        all).  Outputs start as NaN: whatever the kernel leaves unwritten shows."""
        Q = np.ascontiguousarray(Q, dtype=float)
        B, M = Q.shape[0], Q.shape[1]
        dQ = None if dQ is None else np.ascontiguousarray(dQ, dtype=float)
        idx = np.arange(self.n_frames, dtype=np.int32) if frames is None else np.ascontiguousarray(frames, dtype=np.int32)
        assert idx.size and idx.min() >= 0 and idx.max() < self.n_frames
        F, nq = len(idx), self.nq
        nan = lambda *shape: np.full(shape, np.nan)
        g = nan(B, M, F, 3, 4) if want_g else None
        vb = None if dQ is None else nan(B, M, F, 6)
        p_dq, vb_ddq = (nan(B, M, F, nq, 3), nan(B, M, F, nq, 6)) if jacobians else (None, None)
        ptr = lambda a: None if a is None else a.ctypes.data
        self.L.emu_frames(self.h, B, M, Q.ctypes.data, int(Q.shape[2] if q_stride is None else q_stride), ptr(dQ),
                          0 if dQ is None else int(dQ.shape[2]), F, idx.ctypes.data, ptr(g), ptr(vb), ptr(p_dq), ptr(vb_ddq), 1 if poison else 0)
        return FrameKinematics(g, vb, p_dq, vb_ddq)
