"""ctypes driver for the host emulation of the per-trajectory parameter kernels (tests/emu_par/emu_par.cpp, compiled on demand
with g++ from trep_amd/csrc/mvi_core.hpp).  EmuParBatch is emu_harness.EmuBatch on that library, plus set_parameters().  Test
infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

import emu_harness

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "emu_par", "libtrepamd_emu_par.so")
        csrc = os.path.join(_ROOT, "trep_amd", "csrc")
        srcs = [os.path.join(_HERE, "emu_par", "emu_par.cpp")] + [os.path.join(csrc, f) for f in ("mvi_core.hpp", "lanes.hpp", "program.hpp", "devprog_fields.def", "schedule.hpp", "bbd.hpp", "dual.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, srcs[0]], check=True)
        L = ctypes.CDLL(so)
        L.emu_create.restype = ctypes.c_void_p
        L.emu_create.argtypes = [ctypes.c_void_p]
        L.emu_destroy.argtypes = [ctypes.c_void_p]
        L.emu_run.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.emu_set_parameters.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        L.emu_base_row.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        _LIB = L
    return _LIB


class EmuParBatch(emu_harness.EmuBatch):
    def __init__(self, desc, batch, tolerance=1e-10):
        emu_harness.EmuBatch.__init__(self, desc, batch, tolerance)
        self.L.emu_destroy(self.h)
        self.L = lib()
        self.h = self.L.emu_create(ctypes.addressof(desc.struct))
        assert self.h
        self.n_bodies = int(desc.n_masses)

    def base_row(self):
        row = np.zeros(4 * self.n_bodies + 3 + self.nd)
        self.L.emu_base_row(self.h, row.ctypes.data)
        return row

    def set_parameters(self, rows, group, inertia=None, gravity=None, damping=None):
        """Complete rows from the given blocks (None: the system's values), as tg_batch_set_parameters makes them."""
        nb = 4 * self.n_bodies
        table = np.tile(self.base_row(), (rows, 1))
        if inertia is not None:
            table[:, :nb] = np.asarray(inertia, dtype=float).reshape(rows, nb)
        if gravity is not None:
            table[:, nb:nb + 3] = np.asarray(gravity, dtype=float).reshape(rows, 3)
        if damping is not None:
            table[:, nb + 3:] = np.asarray(damping, dtype=float).reshape(rows, self.nd)
        self._table = np.ascontiguousarray(table)
        self.L.emu_set_parameters(self.h, rows, group, self._table.ctypes.data)

    def clear_parameters(self):
        self.L.emu_set_parameters(self.h, 0, 1, None)
