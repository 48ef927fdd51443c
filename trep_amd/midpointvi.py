"""MidpointVI: the midpoint variational integrator, executed on the MI355X.

``BatchMidpointVI`` advances B independent trajectories of one ``System`` at
once on a HIP device; ``MidpointVI`` is the B = 1 shell that keeps the reference
API (/root/reference/trep/midpointvi.py:19-332: initialize_from_state /
initialize_from_configs / step / calc_f, the t/q/p/u/lambda properties, v2) so
the reference's example scripts run unmodified against this package.

All numerical work happens in libtrepamd.so (HIP, gfx950) through the C ABI of
include/trep_amd.h.  State lives in device memory; the properties copy it
in/out.  There is no CPU execution path: without the library or without a GPU
every call raises.
"""
import collections
import os

import numpy as np

from . import _lib
from .descriptor import flatten
from .errors import ConvergenceError

Projection = collections.namedtuple("Projection", "Q dQ mu iterations status")      # BatchMidpointVI.satisfy_constraints
Equilibrium = collections.namedtuple("Equilibrium", "Q mu V iterations status")     # BatchMidpointVI.minimize_potential_energy


class NormalModes(collections.namedtuple("NormalModes", "omega2 modes count rank mu residual sweeps status")):      # BatchMidpointVI.normal_modes
    """omega2 [B][nF] ascending, modes [B][nF][nq], count, rank [B], mu [B][nc], residual [B], sweeps, status [B]; rows beyond
    count are zero."""
    __slots__ = ()

    @property
    def frequencies(self):
        """Natural frequencies in Hz, [B][nF] (formed on the host): NaN where omega2 < 0 (an unstable direction has none)."""
        w2 = np.asarray(self.omega2, dtype=float)
        return np.sqrt(np.where(w2 >= 0.0, w2, np.nan)) / (2.0 * np.pi)

    @property
    def unstable(self):
        """[B]: the number of negative omega2 of every pose (formed on the host); 0 for a minimum of the potential."""
        return (np.asarray(self.omega2) < 0.0).sum(axis=1).astype(np.int32)
StaticResponse = collections.namedtuple("StaticResponse", "dq dmu compliance reaction rank mu residual defect status")      # BatchMidpointVI.static_response
InverseDynamics = collections.namedtuple("InverseDynamics", "U lam P rho h status")     # BatchMidpointVI.inverse_dynamics
FrameKinematics = collections.namedtuple("FrameKinematics", "g vb p_dq vb_ddq")         # BatchMidpointVI.frame_kinematics
TapeMeasures = collections.namedtuple("TapeMeasures", "length velocity length_dq velocity_dq length_dqdq")      # BatchMidpointVI.tape_measures
DynamicsInverse = collections.namedtuple("DynamicsInverse", "U lam rho tau acc status")     # BatchMidpointVI.dynamics_inverse
# ... and what the two inverse questions return with rcond=: the rank of every state or step as one more field
InverseDynamicsRank = collections.namedtuple("InverseDynamicsRank", "U lam P rho h status rank")
DynamicsInverseRank = collections.namedtuple("DynamicsInverseRank", "U lam rho tau acc status rank")
# ... and with bounds=: active (-1 at the lower bound, +1 at the upper, 0 free) and solves (least-squares solves taken) behind rank
InverseDynamicsBounded = collections.namedtuple("InverseDynamicsBounded", "U lam P rho h status rank active solves")
DynamicsInverseBounded = collections.namedtuple("DynamicsInverseBounded", "U lam rho tau acc status rank active solves")


class BatchMidpointVI(object):
    """B trajectories of ``system`` on HIP device ``device`` (state arrays are [B][width])."""

    def __init__(self, system, batch, tolerance=1e-10, device=0, specialize="auto"):
        """specialize: "auto" (default) uses a system-specialised rollout kernel if one has been built for this system
        (trep_amd/specialize.py; never compiles implicitly), True builds one if needed, False keeps the generic kernel."""
        self._system = system
        self._specialize_mode = specialize
        self._specialized = None
        self._batch = int(batch)
        self._device = int(device)
        self._L = _lib.lib()
        _lib.require_device()
        self._desc = flatten(system)
        self._structure_version = system._structure_version
        self._sys_h = self._L.tg_system_create(self._desc.byref())
        if not self._sys_h:
            raise _lib.LibraryError(self._L.tg_last_error().decode())
        self._h = self._L.tg_batch_create(self._sys_h, self._batch, self._device)
        if not self._h:
            msg = self._L.tg_last_error().decode()
            self._L.tg_system_destroy(self._sys_h)
            self._sys_h = None
            raise _lib.LibraryError(msg)
        self.tolerance = tolerance
        self._owned_dev = []
        if specialize is True:
            self.specialize(build=True)
        elif specialize == "auto" and os.environ.get("TREPAMD_NO_SPECIALIZE") is None:
            self.specialize(build=False)

    def specialize(self, build=True):
        """Use a rollout kernel compiled for exactly this system (trep_amd/specialize.py): same results, fewer
        instructions.  With build=False only an already cached specialisation is used (returns False if there is
        none).  A later structure / parameter change of the system drops back to the generic kernel."""
        from . import specialize as _spec
        if not build and not _spec.is_built(self._system):
            return False
        path = os.environ.get("TREPAMD_SPEC_OVERRIDE") or _spec.build(self._system)   # override: A/B experiments only
        _lib.check(self._L.tg_batch_load_specialized(self._h, path.encode()))
        self._specialized = path
        return True

    def refresh(self):
        """Re-flatten the system if it changed since the device program was built.  The reference treats parameter
        writes (Gravity.gravity, spring constants, damping, Distance.distance ...) as plain attribute updates and its
        integrator keeps its state across them (trep/potentials/gravity.py, trep/midpointvi.py:25-136 only
        re-allocates on *structure* changes); here every change re-builds the few-kB device schedule, and the batch
        state (times, q1, q2, p1, p2, u1, lambda1, tolerance, predictor) is carried over whenever the sizes are
        unchanged.  A per-trajectory parameter table (set_parameters) is dropped by a rebuild: its sizes and base values
        belong to the old schedule.  Returns True if a rebuild happened."""
        if self._structure_version == self._system._structure_version:
            return False
        old_sizes = (self.nq, self.nd, self.nk, self.nu, self.nc)
        desc = flatten(self._system)
        sys_h = self._L.tg_system_create(desc.byref())
        if not sys_h:
            raise _lib.LibraryError(self._L.tg_last_error().decode())
        h = self._L.tg_batch_create(sys_h, self._batch, self._device)
        if not h:
            msg = self._L.tg_last_error().decode()
            self._L.tg_system_destroy(sys_h)
            raise _lib.LibraryError(msg)
        keep = None
        if old_sizes == (int(desc.n_configs), int(desc.n_dyn), int(desc.n_kin), int(desc.n_inputs), int(desc.n_constraints)):
            keep = (self.times(), [getattr(self, n) for n in ("q1", "q2", "p1", "p2", "u1", "lambda1")], self.tolerance,
                    self.predictor, self.exact_pivot)
        self._L.tg_batch_destroy(self._h)
        self._L.tg_system_destroy(self._sys_h)
        self._desc, self._sys_h, self._h = desc, sys_h, h
        self._parameter_rows = 0
        self._structure_version = self._system._structure_version
        self._specialized = None
        if self._specialize_mode is True or (self._specialize_mode == "auto" and os.environ.get("TREPAMD_NO_SPECIALIZE") is None):
            self.specialize(build=False)      # a cached specialisation of the NEW schedule, if there is one
        if keep is not None:
            (t1, t2), fields, tol, pred, exact = keep
            self.set_times(t1, t2)
            for n, v in zip(("q1", "q2", "p1", "p2", "u1", "lambda1"), fields):
                setattr(self, n, v)
            self.tolerance = tol
            self.predictor = pred
            self.exact_pivot = exact
        ss = getattr(self, "_step_sizes", None)
        if ss is not None:
            self.set_step_sizes(ss[0], ss[1])
        return True

    def close(self):
        if getattr(self, "_h", None):
            for p in self._owned_dev:
                self._L.tg_device_free(self._device, p)
            self._owned_dev = []
            self._L.tg_batch_destroy(self._h)
            self._h = None
        if getattr(self, "_sys_h", None):
            self._L.tg_system_destroy(self._sys_h)
            self._sys_h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_step_sizes(self, dts=None, by_trajectory=False):
        """Non-uniform time base (include/trep_amd.h, tg_batch_set_step_sizes): `dts` replaces the scalar dt of the rollouts
        (step k uses dts[k]) or, with by_trajectory, of a one-step batch (trajectory t uses dts[t % len(dts)]).  None clears.
        A refused list (a zero or non-finite entry: LibraryError) leaves the list set before in place.  A by-step list leaves
        step() alone; a by-trajectory list applies to every mode (calc_p2 of initialize_from_configs included: set it after) and
        refuses rollouts of more than one step."""
        if dts is None:
            _lib.check(self._L.tg_batch_set_step_sizes(self._h, 0, None, 0))
            self._step_sizes = None
            return
        d = np.ascontiguousarray(dts, dtype=np.float64).reshape(-1)
        _lib.check(self._L.tg_batch_set_step_sizes(self._h, len(d), d.ctypes.data, 1 if by_trajectory else 0))
        self._step_sizes = (d.copy(), bool(by_trajectory))

    @staticmethod
    def _dt_argument(dt, n_steps):
        """(scalar dt for the C call, step-size list or None): rollouts accept a scalar or one step size per step."""
        if np.ndim(dt) == 0:
            return float(dt), None
        d = np.ascontiguousarray(dt, dtype=np.float64).reshape(-1)
        if len(d) != n_steps:
            raise ValueError("expected %d step sizes, got %d" % (n_steps, len(d)))
        if np.allclose(d, d[0], rtol=1e-13, atol=0.0):
            return float(d[0]), None
        return float(d[0]), d

    @property
    def exact_pivot(self):
        """False (default): pivot candidates of the Newton solve are ranked in single precision; True: the reference's
        pivot rule bit for bit (include/trep_amd.h, tg_batch_set_pivot_rule), about 9 % slower."""
        return getattr(self, "_exact_pivot", False)

    @exact_pivot.setter
    def exact_pivot(self, value):
        _lib.check(self._L.tg_batch_set_pivot_rule(self._h, 1 if value else 0))
        self._exact_pivot = bool(value)

    # -- sizes ---------------------------------------------------------------------------
    system = property(lambda self: self._system)
    batch = property(lambda self: self._batch)
    device = property(lambda self: self._device)
    nq = property(lambda self: int(self._desc.n_configs))
    nd = property(lambda self: int(self._desc.n_dyn))
    nk = property(lambda self: int(self._desc.n_kin))
    nu = property(lambda self: int(self._desc.n_inputs))
    nc = property(lambda self: int(self._desc.n_constraints))
    nX = property(lambda self: self.nq + self.nd + self.nk)
    nU = property(lambda self: self.nu + self.nk)

    def info(self):
        out = (np.zeros(8, dtype=np.int32))
        _lib.check(self._L.tg_system_info(self._sys_h, out.ctypes.data_as(_lib._c_ip)))
        keys = ["team", "lds_bytes_per_trajectory", "joints", "levels", "bodies", "items", "pairs", "dh_items"]
        d = dict(zip(keys, (int(v) for v in out)))
        # joints of the floating base's translational prefix whose terms the loaded rollout kernel takes in closed form (tg_batch_info;
        # 0: none, or no specialised kernel loaded)
        kout = np.zeros(8, dtype=np.int32)
        _lib.check(self._L.tg_batch_info(self._h, kout.ctypes.data_as(_lib._c_ip)))
        d["fb_n"] = (int(kout[7]) >> 8) & 0xFF
        # joints of translation runs whose world poses the loaded rollout kernel stores directly (likewise)
        d["tr_n"] = (int(kout[7]) >> 16) & 0xFF
        # the loaded rollout kernel carries the q2 poses into a step's first evaluation behind the step edge; the joints without a q2 twin (likewise)
        d["pose_carry"] = bool((int(kout[7]) >> 24) & 1)
        d["n_carry"] = (int(kout[7]) >> 25) & 0xF
        return d

    MODES = {"rollout": 0, "calc_p2": 1, "calc_f": 2, "deriv1": 3, "deriv2z": 4}
    ALL_MODES = dict(MODES, dynamics=5, dynamics_deriv1=6, energy=7, lagrangian=8)

    # -- per-trajectory parameters ------------------------------------------------------
    def parameters(self):
        """The system's own parameter values as the device schedule holds them (tg_system_parameters): dict with inertia
        [n_bodies][4] (mass, Ixx, Iyy, Izz of system.masses), gravity [3] (None without a Gravity potential) and damping [nd]
        (None without a Damping force)."""
        sizes = np.zeros(4, dtype=np.int32)
        _lib.check(self._L.tg_system_parameters(self._sys_h, sizes.ctypes.data, None, None, None))
        inertia = np.zeros((int(sizes[0]), 4))
        gravity, damping = np.zeros(3), np.zeros(int(sizes[1]))
        _lib.check(self._L.tg_system_parameters(self._sys_h, None, inertia.ctypes.data if inertia.size else None, gravity.ctypes.data,
                                                damping.ctypes.data if damping.size else None))
        return {"inertia": inertia, "gravity": gravity if sizes[2] else None, "damping": damping if sizes[3] else None}

    def set_parameters(self, inertia=None, gravity=None, damping=None, group=1):
        """Per-trajectory masses / inertias, gravity and damping (trep_amd/parameters.py has the shapes): trajectory t uses row
        t // group of each block, a block of one row applies to every trajectory, an omitted block keeps the system's values.
        Every later launch -- rollouts, step, calc_p2 / calc_f, deriv1 / linearize, deriv2z, the continuous dynamics, energy and
        Lagrangian -- runs with the table, through the parameter kernels (kernel_info: par_spec_launched / par_generic_launched);
        the forward-mode entry points (*_forward) raise LibraryError while it is set.  Raises ValueError (nothing changed) for
        bad shapes or values.  The schedule is not rebuilt and a loaded specialised library stays in use.  Set the table before
        initialize_from_configs: the initial momenta (calc_p2) depend on the masses."""
        self.refresh()
        from . import parameters as _par
        rows, group, blocks = _par.pack(self._system, self._batch, inertia=inertia, gravity=gravity, damping=damping, group=group)
        p = lambda name: None if blocks[name] is None or blocks[name].size == 0 else blocks[name].ctypes.data
        rc = self._L.tg_batch_set_parameters(self._h, rows, group, p("inertia"), p("gravity"), p("damping"))
        if rc == _lib.ERR_INVALID:
            raise ValueError(self._L.tg_last_error().decode())
        _lib.check(rc)
        self._parameter_rows = rows

    def clear_parameters(self):
        """Back to the system's own parameters (and the default kernels)."""
        _lib.check(self._L.tg_batch_clear_parameters(self._h))
        self._parameter_rows = 0

    @property
    def has_parameters(self):
        return getattr(self, "_parameter_rows", 0) > 0

    def kernel_info(self):
        """Which kernels this batch has launched (tg_batch_info): `spec_modes` = set of mode names with a specialised kernel
        loaded, `spec_launched` / `generic_launched` = mode names that have actually gone through a specialised / generic
        kernel, and the launch counts; `helper_waves` = wavefronts per trajectory in the loaded library's derivative kernels; `fb_n` = joints of the
        translational prefix the loaded rollout kernel has closed forms for; `tr_n` = joints of translation runs whose world poses it stores directly;
        `pose_carry` / `n_carry` = it was compiled to carry the q2 poses into a step's first evaluation behind the step edge / the joints without a q2 twin that needs
        (what the library holds, not a record that a carried evaluation ran: that takes the step-edge path);
        `spec_library` the loaded file.  The par_* keys: the same for the per-trajectory parameter kernels (set_parameters),
        over all kernel modes (ALL_MODES), with `par_spec_launch_mask` / `par_generic_launch_mask` the raw mode bits as
        `spec_launch_mask` / `generic_launch_mask` are for the default kernels (bit 9: the projection, bit 10: the equilibrium search,
        bit 11: inverse dynamics, bit 12: frame kinematics, which have no name in ALL_MODES); `parameter_rows` / `parameter_group` the current table (0: none)."""
        out = np.zeros(8, dtype=np.int32)
        _lib.check(self._L.tg_batch_info(self._h, out.ctypes.data_as(_lib._c_ip)))
        names = lambda bits: sorted(n for n, m in self.MODES.items() if (int(bits) >> m) & 1)
        par = np.zeros(8, dtype=np.int32)
        _lib.check(self._L.tg_batch_par_info(self._h, par.ctypes.data_as(_lib._c_ip)))
        every = lambda bits: sorted(n for n, m in self.ALL_MODES.items() if (int(bits) >> m) & 1)
        return {"spec_modes": names(out[0]), "spec_launched": names(out[1]), "generic_launched": names(out[2]),
                "spec_launch_mask": int(out[1]), "generic_launch_mask": int(out[2]),
                "spec_launches": int(out[3]), "generic_launches": int(out[4]), "exact_pivot": bool(out[5]), "team": int(out[6]),
                "helper_waves": int(out[7]) & 0xFF, "fb_n": (int(out[7]) >> 8) & 0xFF, "tr_n": (int(out[7]) >> 16) & 0xFF,
                "pose_carry": bool((int(out[7]) >> 24) & 1), "n_carry": (int(out[7]) >> 25) & 0xF, "spec_library": self._specialized,
                # per-trajectory parameter kernels (set_parameters); the keys above count the default kernels only
                "par_spec_modes": every(par[0]), "par_spec_launched": every(par[1]), "par_generic_launched": every(par[2]),
                "par_spec_launch_mask": int(par[1]), "par_generic_launch_mask": int(par[2]), "par_spec_launches": int(par[3]), "par_generic_launches": int(par[4]), "parameter_rows": int(par[5]),
                "parameter_group": int(par[6])}

    @property
    def stream(self):
        """The batch's HIP stream (hipStream_t as an integer), e.g. for ``Communicator.wait_stream``."""
        return self._L.tg_batch_stream(self._h)

    # -- state ---------------------------------------------------------------------------
    @property
    def tolerance(self):
        return self._tolerance

    @tolerance.setter
    def tolerance(self, value):
        self._tolerance = float(value)
        _lib.check(self._L.tg_batch_set_tolerance(self._h, self._tolerance))

    def times(self):
        import ctypes
        a, b = ctypes.c_double(), ctypes.c_double()
        _lib.check(self._L.tg_batch_get_times(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def set_times(self, t1, t2):
        _lib.check(self._L.tg_batch_set_times(self._h, float(t1), float(t2)))

    def _get(self, field, width):
        out = np.zeros((self._batch, width))
        if width:
            _lib.check(self._L.tg_batch_get(self._h, field, out.ctypes.data))
        return out

    def _set(self, field, width, value):
        arr = np.ascontiguousarray(np.broadcast_to(np.asarray(value, dtype=np.float64), (self._batch, width)))
        if width:
            _lib.check(self._L.tg_batch_set(self._h, field, arr.ctypes.data))

    def _field(field, width_attr):
        def getter(self):
            return self._get(field, getattr(self, width_attr))

        def setter(self, value):
            self._set(field, getattr(self, width_attr), value)
        return property(getter, setter)

    q1 = _field(_lib.F_Q1, "nq")
    q2 = _field(_lib.F_Q2, "nq")
    p1 = _field(_lib.F_P1, "nd")
    p2 = _field(_lib.F_P2, "nd")
    u1 = _field(_lib.F_U1, "nu")
    lambda1 = _field(_lib.F_LAMBDA1, "nc")
    del _field

    # -- reference semantics, batched -------------------------------------------------------------
    def initialize_from_state(self, t1, q1, p1, lambda1=None):
        """midpointvi.py:138-153: (t2,q2,p2) <- (t1,q1,p1), lambda1 <- given or 0."""
        self.refresh()
        self.set_times(t1, t1)
        self.q1 = q1
        self.p1 = p1
        self.q2 = q1
        self.p2 = p1
        self.lambda1 = np.zeros((self._batch, self.nc)) if lambda1 is None else lambda1

    def initialize_from_configs(self, t0, q0, t1, q1, lambda1=None):
        """midpointvi.py:155-172: p2 = D2L2(q0, q1) computed on the device."""
        self.refresh()
        self.set_times(t0, t1)
        self.q1 = q0
        self.q2 = q1
        _lib.check(self._L.tg_batch_calc_p2(self._h))
        self.lambda1 = np.zeros((self._batch, self.nc)) if lambda1 is None else lambda1

    def calc_p2(self):
        self.refresh()
        _lib.check(self._L.tg_batch_calc_p2(self._h))

    def calc_f(self):
        self.refresh()
        out = np.zeros((self._batch, self.nd + self.nc))
        _lib.check(self._L.tg_batch_calc_f(self._h, out.ctypes.data))
        return out

    # -- first derivatives (reference MidpointVI_calc_deriv1, midpointvi.c:1100-1120) -----------------
    D1_NAMES = ["q2_dq1", "q2_dp1", "q2_du1", "q2_dk2", "p2_dq1", "p2_dp1", "p2_du1", "p2_dk2",
                "l1_dq1", "l1_dp1", "l1_du1", "l1_dk2"]

    def calc_deriv1(self):
        """Compute all twelve first-derivative arrays of the last solved step on the device."""
        self.refresh()
        _lib.check(self._L.tg_batch_deriv1(self._h))

    def deriv1(self, name):
        """[B][derivative variable][output] (the reference's C layout, trep.h:425-437)."""
        k = self.D1_NAMES.index(name)
        rows = (self.nq, self.nd, self.nu, self.nk)[k % 4]
        width = self.nc if k // 4 == 2 else self.nd
        out = np.zeros((self._batch, rows, width))
        if out.size:
            _lib.check(self._L.tg_batch_get(self._h, _lib.F_D1_BASE + k, out.ctypes.data))
        return out

    def deriv2_contract(self, Z, ZL=None):
        """Second derivatives contracted with Z [B][nX] over the output index: HZ [B][R][R] with the
        derivative variables ordered (q1[nq], p1[nd], u1[nu], k2[nk]).  HZ[b][A][B] =
        sum_o Z[b][o] q2_dAdB[A][B][o] + Z[b][nq+o] p2_dAdB[A][B][o] (what DSystem.fdxdx/fdxdu/fdudu use)."""
        self.refresh()
        R = self.nq + self.nd + self.nu + self.nk
        Z = _lib.as_f64(np.broadcast_to(np.asarray(Z, dtype=float), (self._batch, self.nX)), (self._batch, self.nX))
        HZ = np.zeros((self._batch, R, R))
        if ZL is None:
            _lib.check(self._L.tg_batch_deriv2_contract(self._h, Z.ctypes.data, HZ.ctypes.data))
        else:   # additionally sum_c ZL[b][c] * lambda1_dAdB[A][B][c]
            ZL = _lib.as_f64(np.broadcast_to(np.asarray(ZL, dtype=float), (self._batch, self.nc)), (self._batch, self.nc))
            _lib.check(self._L.tg_batch_deriv2_contract_lambda(self._h, Z.ctypes.data, _lib.ptr(ZL), HZ.ctypes.data))
        return HZ

    def step(self, t2, u1=None, k2=None, max_iterations=200, q2_hint=None, lambda1_hint=None):
        """One MidpointVI.step for every trajectory.  Returns (iterations[B], status[B])."""
        self.refresh()
        B = self._batch
        u = None if self.nu == 0 else _lib.as_f64(np.broadcast_to(np.asarray(u1, dtype=float), (B, self.nu)), (B, self.nu))
        k = None if self.nk == 0 else _lib.as_f64(np.broadcast_to(np.asarray(k2, dtype=float), (B, self.nk)), (B, self.nk))
        qh = None if q2_hint is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(q2_hint, dtype=float)[..., :self.nd], (B, self.nd)))
        lh = None if lambda1_hint is None or self.nc == 0 else _lib.as_f64(
            np.broadcast_to(np.asarray(lambda1_hint, dtype=float), (B, self.nc)), (B, self.nc))
        iters = np.zeros(B, dtype=np.int32)
        status = np.zeros(B, dtype=np.int32)
        _lib.check(self._L.tg_batch_step(self._h, float(t2), _lib.ptr(u), _lib.ptr(k), _lib.ptr(qh), _lib.ptr(lh),
                                         int(max_iterations), iters.ctypes.data, status.ctypes.data))
        return iters, status

    # -- device-resident rollouts ------------------------------------------------------------------
    def device_array(self, host):
        """Upload a host array; returns a device pointer owned by this batch."""
        host = np.ascontiguousarray(host, dtype=np.float64)
        p = self._L.tg_device_alloc(self._device, max(host.nbytes, 8))
        if not p:
            raise _lib.LibraryError(self._L.tg_last_error().decode())
        if host.nbytes:
            _lib.check(self._L.tg_memcpy_h2d(self._device, p, host.ctypes.data, host.nbytes))
        self._owned_dev.append(p)
        return p

    def device_empty(self, n_doubles):
        p = self._L.tg_device_alloc(self._device, max(8 * int(n_doubles), 8))
        if not p:
            raise _lib.LibraryError(self._L.tg_last_error().decode())
        self._owned_dev.append(p)
        return p

    def download(self, dev_ptr, shape):
        out = np.zeros(shape)
        if out.nbytes:
            _lib.check(self._L.tg_memcpy_d2h(self._device, out.ctypes.data, dev_ptr, out.nbytes))
        return out

    def rollout_device(self, n_steps, dt, U_dev=None, K_dev=None, X_dev=None, max_iterations=200):
        """Asynchronous n_steps-step rollout entirely on the device (one kernel launch)."""
        self.refresh()
        _lib.check(self._L.tg_batch_rollout(self._h, int(n_steps), float(dt), U_dev, K_dev, X_dev,
                                            int(max_iterations)))

    def rollout(self, n_steps, dt, U=None, K=None, max_iterations=200):
        """Convenience: upload U [B][N][nu] / K [B][N][nk], roll out, download X [B][N+1][nX].  `dt` is a scalar or one step
        size per step (non-uniform time base)."""
        self.refresh()
        dt, dts = self._dt_argument(dt, n_steps)
        if dts is not None:
            saved = getattr(self, "_step_sizes", None)
            self.set_step_sizes(dts)
            try:
                return self.rollout(n_steps, dt, U, K, max_iterations)
            finally:
                self.set_step_sizes(*(saved if saved is not None else (None,)))
        B = self._batch
        U_dev = self.device_array(_lib.as_f64(U, (B, n_steps, self.nu))) if self.nu else None
        K_dev = self.device_array(_lib.as_f64(K, (B, n_steps, self.nk))) if self.nk else None
        X_dev = self.device_empty(B * (n_steps + 1) * self.nX)
        self.rollout_device(n_steps, dt, U_dev, K_dev, X_dev, max_iterations)
        self.synchronize()
        X = self.download(X_dev, (B, n_steps + 1, self.nX))
        for p in (U_dev, K_dev, X_dev):
            if p:
                self._L.tg_device_free(self._device, p)
                self._owned_dev.remove(p)
        return X

    def rollout_closed_loop(self, n_steps, dt, Kproj, bX, bU, group_size=1, max_iterations=200):
        """Projection-operator rollout: U_k = bU_k - Kproj_k (X_k - bX_k) evaluated in the kernel.
        Kproj [groups][N][nU][nX], bX [B][N+1][nX], bU [B][N][nU] (host arrays); returns (X, U).  `dt`: scalar or one step
        size per step."""
        self.refresh()
        dt, dts = self._dt_argument(dt, n_steps)
        if dts is not None:
            saved = getattr(self, "_step_sizes", None)
            self.set_step_sizes(dts)
            try:
                return self.rollout_closed_loop(n_steps, dt, Kproj, bX, bU, group_size, max_iterations)
            finally:
                self.set_step_sizes(*(saved if saved is not None else (None,)))
        B, nX, nU = self._batch, self.nX, self.nU
        groups = (B + group_size - 1) // group_size
        K_dev = self.device_array(_lib.as_f64(Kproj, (groups, n_steps, nU, nX)))
        bX_dev = self.device_array(_lib.as_f64(bX, (B, n_steps + 1, nX)))
        bU_dev = self.device_array(_lib.as_f64(bU, (B, n_steps, nU)))
        X_dev = self.device_empty(B * (n_steps + 1) * nX)
        U_dev = self.device_empty(B * n_steps * nU)
        _lib.check(self._L.tg_batch_rollout_closed_loop(self._h, int(n_steps), float(dt), K_dev, int(group_size),
                                                        bX_dev, bU_dev, X_dev, U_dev, int(max_iterations)))
        self.synchronize()
        X = self.download(X_dev, (B, n_steps + 1, nX))
        U = self.download(U_dev, (B, n_steps, nU))
        for p in (K_dev, bX_dev, bU_dev, X_dev, U_dev):
            self._L.tg_device_free(self._device, p)
            self._owned_dev.remove(p)
        return X, U

    def dynamics(self, Q, dQ, U=None, ddQk=None):
        """Continuous dynamics of B states at once (the reference's System.f() / System.lambda_(), system.py:951-1024):
        Q, dQ [B][nq]; U [B][nu]; ddQk [B][nk] accelerations of the kinematic configs (zeros when omitted).
        Returns (ddq [B][nd], lambda [B][nc], status [B]).  The integrator state is left alone."""
        self.refresh()
        B = self._batch
        Q = _lib.as_f64(np.broadcast_to(np.asarray(Q, dtype=float), (B, self.nq)), (B, self.nq))
        dQ = _lib.as_f64(np.broadcast_to(np.asarray(dQ, dtype=float), (B, self.nq)), (B, self.nq))
        U = np.zeros((B, self.nu)) if U is None else _lib.as_f64(np.broadcast_to(np.asarray(U, dtype=float), (B, self.nu)), (B, self.nu))
        K = np.zeros((B, self.nk)) if ddQk is None else _lib.as_f64(np.broadcast_to(np.asarray(ddQk, dtype=float), (B, self.nk)), (B, self.nk))
        ddq, lam = np.zeros((B, self.nd)), np.zeros((B, self.nc))
        status = np.zeros(B, dtype=np.int32)
        _lib.check(self._L.tg_batch_dynamics(self._h, _lib.ptr(Q), _lib.ptr(dQ), _lib.ptr(U), _lib.ptr(K),
                                             _lib.ptr(ddq), _lib.ptr(lam), status.ctypes.data))
        return ddq, lam, status

    def _box(self, bounds):
        """bounds = (lo, hi) -> contiguous lo, hi [rows][nu + nc] and rows (1 or B): each side None (no bound), a scalar, [n] or [B][n]
        in (u | lambda) order."""
        B, n = self._batch, self.nu + self.nc
        try:
            lo, hi = bounds
        except (TypeError, ValueError):
            raise ValueError("bounds must be a pair (lo, hi)")
        lo = np.asarray(-np.inf if lo is None else lo, dtype=np.float64)
        hi = np.asarray(np.inf if hi is None else hi, dtype=np.float64)
        for a in (lo, hi):
            if a.ndim > 2 or (a.ndim >= 1 and a.shape[-1] != n) or (a.ndim == 2 and a.shape[0] != B):
                raise ValueError("expected bounds of shape (), (%d,) or (%d, %d), got %r" % (n, B, n, a.shape))
        rows = B if (lo.ndim == 2 or hi.ndim == 2) else 1
        lo = np.ascontiguousarray(np.broadcast_to(lo, (rows, n)), dtype=np.float64)
        hi = np.ascontiguousarray(np.broadcast_to(hi, (rows, n)), dtype=np.float64)
        return lo, hi, rows

    def tension_bounds(self, call="inverse_dynamics"):
        """(lo, hi) [nu + nc] for bounds=: the inputs unbounded and the multiplier of every Distance constraint -- a string --
        confined to the side on which it PULLS its two points together.  The side depends on the call, because the multipliers enter
        the two sets of equations with opposite signs (h = |p1 - p2| - d in both): call="dynamics_inverse" (continuous, +Ad' lambda
        beside the applied forces): lambda <= 0 pulls; call="inverse_dynamics" (discrete, -Dh' lambda; the sign of the integrator's
        lambda1): lambda >= 0 pulls.  Other constraints stay unbounded."""
        if call not in ("dynamics_inverse", "inverse_dynamics"):
            raise ValueError("call must be 'dynamics_inverse' or 'inverse_dynamics', got %r" % (call,))
        n = self.nu + self.nc
        lo, hi = np.full(n, -np.inf), np.full(n, np.inf)
        for c, con in enumerate(self._system.constraints):
            if type(con).__name__ == "Distance":
                if call == "dynamics_inverse":
                    hi[self.nu + c] = 0.0
                else:
                    lo[self.nu + c] = 0.0
        return lo, hi

    def dynamics_inverse(self, Q, dQ, ddQ, ridge=0.0, rcond=None, bounds=None):
        """Computed torque, the inverse of dynamics() (include/trep_amd.h, tg_batch_dynamics_inverse): Q, dQ, ddQ [B][nq] or
        [B][M][nq], kinematic configs included (the kinematic part of ddQ is what dynamics() calls ddQk).  Every state is one
        least-squares solve for (u, lambda), all B x M of them in one launch.  Returns the namedtuple (U [B][M][nu], lam [B][M][nc],
        rho [B][M][nd], tau [B][M][nd], acc [B][M][nc], status [B][M]): tau is the generalized force the motion needs from inputs and
        constraints together, rho the part of it they cannot supply (zero for accelerations dynamics() returned), acc how far ddQ is
        from consistent with the constraints.  status: TG_OK, or TG_SINGULAR where the solver rejected the state (U, lam, rho zero
        there).  ridge >= 0 weighs |(u, lambda)|^2 against |rho|^2; it is required (ValueError) when nu + nc > nd, and a
        rank-deficient system needs it too -- that is not detected.  For inputs [B][nq] the M axis is dropped.  With a parameter
        table each trajectory uses its row; the time base has no say.  The integrator state of the batch is left alone.
        rcond (a float in [0, 1); None: the path above, unchanged) answers by rank-revealing least squares instead
        (tg_batch_dynamics_inverse_lsq): (u, lambda) is numpy.linalg.lstsq's minimum-norm answer on [A; sqrt(ridge) I], so a
        rank-deficient system needs no ridge and nu + nc > nd is accepted without one; pivot columns with a norm <= rcond times the
        first one's count as dependent.  The namedtuple then has rank [B][M] as an additional last field: the number of independent
        force directions of each state (with ridge > 0: of the stacked block).
        bounds = (lo, hi) (None: the paths above, unchanged) confines (u | lambda) to a box and answers with the exact minimiser
        of |rho|^2 + ridge |z|^2 inside it (tg_batch_dynamics_inverse_bounded; an active-set loop around the rank-revealing solve,
        scipy.optimize.lsq_linear(method="bvls")'s method).  lo and hi are [nu + nc] or [B][nu + nc] in (u | lambda) order, a scalar
        broadcasts, None on one side or +-inf per variable mean no bound; rcond then defaults to 1e-9.  A state whose unbounded answer
        lies in the box returns that answer's bits.  rho now holds what inputs and constraints cannot supply WITHIN the box.  The
        namedtuple has active [B][M][nu + nc] (-1 at the lower bound, +1 at the upper, 0 free; lo == hi reports -1) and solves [B][M]
        behind rank (the first solve's).  A state whose first solve loses rank has no unique minimiser: TG_SINGULAR -- use a ridge;
        nu + nc > nd without one is refused (ValueError).  A string (Distance constraint) pulls where lambda <= 0 HERE:
        tension_bounds("dynamics_inverse")."""
        self.refresh()
        B, nq = self._batch, self.nq
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        flat = Q.ndim == 2
        if flat:
            Q = Q[:, None, :]
        if Q.ndim != 3 or Q.shape[0] != B or Q.shape[1] < 1 or Q.shape[2] != nq:
            raise ValueError("expected Q of shape (%d, %d) or (%d, M, %d) with M >= 1, got %r" % (B, nq, B, nq, Q.shape))
        M = Q.shape[1]

        def like_q(a, name):
            if a is None:
                raise ValueError("%s is required" % name)
            a = np.ascontiguousarray(a, dtype=np.float64)
            return _lib.as_f64(a[:, None, :] if flat and a.ndim == 2 else a, (B, M, nq))
        dQ, ddQ = like_q(dQ, "dQ"), like_q(ddQ, "ddQ")
        U, lam, rho = np.zeros((B, M, self.nu)), np.zeros((B, M, self.nc)), np.zeros((B, M, self.nd))
        tau, acc, status = np.zeros((B, M, self.nd)), np.zeros((B, M, self.nc)), np.zeros((B, M), dtype=np.int32)
        rank = np.zeros((B, M), dtype=np.int32)
        if bounds is not None:
            lo, hi, rows = self._box(bounds)
            active, solves = np.zeros((B, M, self.nu + self.nc), dtype=np.int32), np.zeros((B, M), dtype=np.int32)
            rc = self._L.tg_batch_dynamics_inverse_bounded(self._h, M, Q.ctypes.data, dQ.ctypes.data, ddQ.ctypes.data, float(ridge),
                                                           float(1e-9 if rcond is None else rcond), _lib.ptr(lo), _lib.ptr(hi), rows,
                                                           _lib.ptr(U), _lib.ptr(lam), _lib.ptr(rho), _lib.ptr(tau), _lib.ptr(acc),
                                                           _lib.ptr(active), solves.ctypes.data, rank.ctypes.data, status.ctypes.data)
        elif rcond is None:
            rc = self._L.tg_batch_dynamics_inverse(self._h, M, Q.ctypes.data, dQ.ctypes.data, ddQ.ctypes.data, float(ridge), _lib.ptr(U),
                                                   _lib.ptr(lam), _lib.ptr(rho), _lib.ptr(tau), _lib.ptr(acc), status.ctypes.data)
        else:
            rc = self._L.tg_batch_dynamics_inverse_lsq(self._h, M, Q.ctypes.data, dQ.ctypes.data, ddQ.ctypes.data, float(ridge), float(rcond),
                                                       _lib.ptr(U), _lib.ptr(lam), _lib.ptr(rho), _lib.ptr(tau), _lib.ptr(acc),
                                                       rank.ctypes.data, status.ctypes.data)
        if rc == _lib.ERR_INVALID:
            raise ValueError(self._L.tg_last_error().decode())
        _lib.check(rc)
        drop = (lambda a: a[:, 0]) if flat else (lambda a: a)
        if bounds is not None:
            return DynamicsInverseBounded(drop(U), drop(lam), drop(rho), drop(tau), drop(acc), drop(status), drop(rank), drop(active), drop(solves))
        if rcond is None:
            return DynamicsInverse(drop(U), drop(lam), drop(rho), drop(tau), drop(acc), drop(status))
        return DynamicsInverseRank(drop(U), drop(lam), drop(rho), drop(tau), drop(acc), drop(status), drop(rank))

    def dynamics_inverse_device(self, n_states, Q_dev, dQ_dev, ddQ_dev, q_row_stride=None, dq_row_stride=None, ddq_row_stride=None,
                                ridge=0.0, U_dev=None, lam_dev=None, rho_dev=None, tau_dev=None, acc_dev=None, status_dev=None,
                                rcond=None, rank_dev=None, bounds_dev=None, active_dev=None, solves_dev=None):
        """dynamics_inverse on device pointers, asynchronous on the batch's stream (tg_batch_dynamics_inverse_device).  Row (b, m) is
        read at Q_dev + (b n_states + m) q_row_stride doubles (dQ_dev and ddQ_dev likewise with their own strides): the default nq
        for packed arrays, nX to read the configurations straight from a rollout's X [B][n_states][nX].  The outputs are laid out as
        dynamics_inverse returns them ([B][n_states]...); any may be None.  rcond (None: the path above): the rank-revealing path
        (tg_batch_dynamics_inverse_lsq_device), with rank_dev int32 [B][n_states] or None.  bounds_dev = (lo_dev, hi_dev, rows): the
        bounded path (tg_batch_dynamics_inverse_bounded_device) with device arrays [rows][nu + nc], rows 1 or B, whose contents are
        taken on trust (numbers, lo <= hi); rcond defaults to 1e-9; active_dev int32 [B][n_states][nu + nc], solves_dev int32
        [B][n_states], each or None."""
        self.refresh()
        nq = self.nq
        strides = (int(nq if q_row_stride is None else q_row_stride), int(nq if dq_row_stride is None else dq_row_stride),
                   int(nq if ddq_row_stride is None else ddq_row_stride))
        if bounds_dev is None and (active_dev is not None or solves_dev is not None):
            raise ValueError("active_dev and solves_dev need bounds_dev")
        if bounds_dev is not None:
            lo_dev, hi_dev, rows = bounds_dev
            rc = self._L.tg_batch_dynamics_inverse_bounded_device(self._h, int(n_states), Q_dev, strides[0], dQ_dev, strides[1], ddQ_dev,
                                                                  strides[2], float(ridge), float(1e-9 if rcond is None else rcond), lo_dev,
                                                                  hi_dev, int(rows), U_dev, lam_dev, rho_dev, tau_dev, acc_dev, active_dev,
                                                                  solves_dev, rank_dev, status_dev)
        elif rcond is None:
            if rank_dev is not None:
                raise ValueError("rank_dev needs rcond")
            rc = self._L.tg_batch_dynamics_inverse_device(self._h, int(n_states), Q_dev, strides[0], dQ_dev, strides[1], ddQ_dev, strides[2],
                                                          float(ridge), U_dev, lam_dev, rho_dev, tau_dev, acc_dev, status_dev)
        else:
            rc = self._L.tg_batch_dynamics_inverse_lsq_device(self._h, int(n_states), Q_dev, strides[0], dQ_dev, strides[1], ddQ_dev, strides[2],
                                                              float(ridge), float(rcond), U_dev, lam_dev, rho_dev, tau_dev, acc_dev, rank_dev,
                                                              status_dev)
        if rc == _lib.ERR_INVALID:
            raise ValueError(self._L.tg_last_error().decode())
        _lib.check(rc)

    def free_mask(self, keep_kinematic=False, constant_q_list=None):
        """int32 [nq], 1 = free: the configs System.satisfy_constraints would move (reference trep/system.py:176-186) -- everything
        outside constant_q_list (names or Config objects) if one is given, else the dynamic configs with keep_kinematic, else all."""
        configs = self._system.configs
        if constant_q_list:
            fixed = set(self._system.get_config(c).name for c in constant_q_list)
            return np.array([0 if c.name in fixed else 1 for c in configs], dtype=np.int32)
        if keep_kinematic:
            return np.array([0 if c.kinematic else 1 for c in configs], dtype=np.int32)
        return np.ones(len(configs), dtype=np.int32)

    def _pose_call(self, Q, keep_kinematic, constant_q_list):
        """What the pose solvers share before their call: the batch refreshed, Q broadcast to [B][nq], the free mask (None: every
        config) and the outputs every one of them has.  Returns (Q, free, q, mu, iterations, status)."""
        self.refresh()
        B = self._batch
        Q = _lib.as_f64(np.broadcast_to(np.asarray(Q, dtype=float), (B, self.nq)), (B, self.nq))
        free = None if not (keep_kinematic or constant_q_list) else self.free_mask(keep_kinematic, constant_q_list)
        q, mu = np.zeros((B, self.nq)), np.zeros((B, self.nc))
        iters, status = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        return Q, free, q, mu, iters, status

    def satisfy_constraints(self, Q, dQ=None, tolerance=1e-10, keep_kinematic=False, constant_q_list=None, max_iterations=50):
        """System.satisfy_constraints (reference trep/system.py:158-214) for B poses in one launch: every Q[b] moves to the nearest
        pose (least squares over the free configs; the others keep their values) with h(q) = 0, by Newton on the KKT conditions
        (include/trep_amd.h, tg_batch_project_constraints).  Q [B][nq]; dQ [B][nq], optional: rates made tangent to the constraints
        at the new pose, the fixed configs' rates kept.  Returns the namedtuple (Q, dQ, mu, iterations, status): [B][nq], [B][nq] or
        None, [B][nc] multipliers, [B] Newton steps, [B] TG_OK / TG_NOT_CONVERGED (q = the last iterate) / TG_SINGULAR (q = the
        iterate before the rejected solve).  Nothing is raised for a trajectory that fails: look at status.  The system's own
        configuration and the integrator state of the batch are left alone."""
        Q, free, q, mu, iters, status = self._pose_call(Q, keep_kinematic, constant_q_list)
        B = self._batch
        dQ = None if dQ is None else _lib.as_f64(np.broadcast_to(np.asarray(dQ, dtype=float), (B, self.nq)), (B, self.nq))
        dq = None if dQ is None else np.zeros((B, self.nq))
        _lib.check(self._L.tg_batch_project_constraints(self._h, _lib.ptr(Q), _lib.ptr(dQ), None if free is None else free.ctypes.data,
                                                        float(tolerance), int(max_iterations), _lib.ptr(q), _lib.ptr(dq), _lib.ptr(mu),
                                                        iters.ctypes.data, status.ctypes.data))
        return Projection(q, dq, mu, iters, status)

    def minimize_potential_energy(self, Q, tolerance=1e-10, keep_kinematic=False, constant_q_list=None, max_iterations=100):
        """System.minimize_potential_energy (reference trep/system.py:215-272) for B poses in one launch: every Q[b] moves to a
        minimum of the potential energy over the free configs (the others keep their values bit for bit) with h(q) = 0, by a
        safeguarded Newton iteration on the KKT conditions (include/trep_amd.h, tg_batch_minimize_potential).  With a parameter
        table (set_parameters) each pose rests under its own row's masses, inertias and gravity.  Q [B][nq].  Returns the
        namedtuple (Q, mu, V, iterations, status): [B][nq], [B][nc] multipliers, [B][2] the potential at the start and at the
        returned pose, [B] trials, [B] TG_OK / TG_NOT_CONVERGED (q = the last accepted iterate) / TG_SINGULAR (the
        regularisation ran out).  Nothing is raised for a pose that fails: look at status.  The system's own configuration and
        the integrator state of the batch are left alone."""
        Q, free, q, mu, iters, status = self._pose_call(Q, keep_kinematic, constant_q_list)
        v = np.zeros((self._batch, 2))
        _lib.check(self._L.tg_batch_minimize_potential(self._h, _lib.ptr(Q), None if free is None else free.ctypes.data, float(tolerance),
                                                       int(max_iterations), _lib.ptr(q), _lib.ptr(mu), _lib.ptr(v), iters.ctypes.data,
                                                       status.ctypes.data))
        return Equilibrium(q, mu, v, iters, status)

    def normal_modes(self, Q, mu=None, constant_q_list=None, rcond=1e-9, max_sweeps=30):
        """Natural frequencies and mode shapes of B poses in one launch (include/trep_amd.h, tg_batch_normal_modes): per pose the
        eigenproblem K phi = omega^2 M phi on the tangent space of the constraints, over the free configs -- every dynamic config
        outside constant_q_list (names or Config objects); a kinematic config is never free.  K = V_qq + sum_c mu_c h_c,qq and M = L_ddqddq at rest; with a
        parameter table (set_parameters) each pose under its own row's masses, inertias and gravity.  Q [B][nq].  mu [B][nc]: the
        constraints' multipliers at the pose, for example those minimize_potential_energy returned; None: the least-squares
        multipliers under rcond.  Returns the namedtuple NormalModes(omega2 [B][nF] ascending, modes [B][nF][nq] -- M-orthonormal,
        tangent to the constraints, zero at the held configs, the component of largest magnitude positive --, count [B] = nF - rank,
        rank [B] of Dh over the free configs, mu [B][nc], residual [B] = |V_q + Dh' mu|inf over the free configs, sweeps [B], status
        [B]); rows beyond count are zero.  .frequencies (Hz, NaN where omega2 < 0) and .unstable (negative omega2 per pose) are
        formed on the host.  A pose with residual > 0 is not at rest: its modes are those of the motion linearised with the
        unbalanced force frozen, i.e. of the quadratic model of V + mu.h at that pose -- meaningful only as far as the residual is
        small.  status: TG_OK; TG_NOT_CONVERGED the Jacobi sweeps ran out (the current answer is returned); TG_SINGULAR the reduced
        mass matrix is not positive definite (a massless free config) or the pose is not finite: every output of that pose is
        zero.  Nothing is raised for a pose that fails.  The integrator state of the batch is left alone."""
        self.refresh()
        B = self._batch
        Q = _lib.as_f64(np.broadcast_to(np.asarray(Q, dtype=float), (B, self.nq)), (B, self.nq))
        free = np.array([0 if c.kinematic else 1 for c in self._system.configs], dtype=np.int32)
        if constant_q_list:
            free &= self.free_mask(False, constant_q_list)
        nF = int(free.sum())
        mu_in = None if mu is None else _lib.as_f64(np.broadcast_to(np.asarray(mu, dtype=float), (B, self.nc)), (B, self.nc))
        omega2, modes = np.zeros((B, nF)), np.zeros((B, nF, self.nq))
        count, rank = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        mu_out, residual = np.zeros((B, self.nc)), np.zeros(B)
        sweeps, status = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        rc = self._L.tg_batch_normal_modes(self._h, _lib.ptr(Q), _lib.ptr(mu_in), free.ctypes.data, float(rcond), int(max_sweeps),
                                           omega2.ctypes.data, modes.ctypes.data, count.ctypes.data, rank.ctypes.data, _lib.ptr(mu_out),
                                           residual.ctypes.data, sweeps.ctypes.data, status.ctypes.data)
        if rc == _lib.ERR_INVALID:
            raise ValueError(self._L.tg_last_error().decode())
        _lib.check(rc)
        return NormalModes(omega2, modes, count, rank, mu_out, residual, sweeps, status)

    def _response_sets(self, keep_kinematic, constant_q_list, drive):
        """(free [nq] int32, drive [nD] int32) of a static_response call: the mask as minimize_potential_energy builds it, the
        driven configs (names or Config objects; None: every held config, in config order) as places in system.configs."""
        free = np.ascontiguousarray(self.free_mask(keep_kinematic, constant_q_list), dtype=np.int32)
        if drive is None:
            places = np.flatnonzero(free == 0)
        else:
            names = [c.name for c in self._system.configs]
            places = [names.index(self._system.get_config(c).name) for c in drive]
        return free, np.ascontiguousarray(places, dtype=np.int32)

    def static_response(self, Q, mu=None, keep_kinematic=False, constant_q_list=None, drive=None, compliance=True, rcond=1e-9):
        """How B rest poses and their constraint forces answer a moved held config and a load, in one launch (include/trep_amd.h,
        tg_batch_static_response).  keep_kinematic and constant_q_list mean what they mean for minimize_potential_energy -- pass the
        same ones: they pick the free configs F, every other config is held.  drive: names or Config objects among the held
        configs; None: all of them, in config order.  Q [B][nq]: the poses, for example those minimize_potential_energy returned;
        mu [B][nc]: their multipliers, None: the least-squares multipliers under rcond.  With a parameter table (set_parameters)
        each pose under its own row's masses and gravity.  Returns the namedtuple StaticResponse(dq [B][nD][nq]: row j the
        derivative of the rest pose along driven config j -- 1 at its own place, 0 at the other held configs --, dmu [B][nD][nc]
        the multipliers' derivative, compliance [B][nq][nq]: a generalized force f on the free configs moves the pose by C f,
        reaction [B][nq][nc]: and the multipliers by R'f (both zero at the held configs; None without compliance=True), rank [B]
        of Dh over the free configs, mu [B][nc], residual [B] = |V_q + Dh' mu|inf over the free configs, defect [B] =
        |Dh dq|inf, non-zero only where the constraints cannot follow the drive, status [B]).  status: TG_OK; TG_SINGULAR the
        pose is not a strict minimum on the tangent space of the constraints (or is not finite): every output of that pose is
        zero.  Nothing is raised for a pose that fails.  The integrator state of the batch is left alone."""
        self.refresh()
        B = self._batch
        Q = _lib.as_f64(np.broadcast_to(np.asarray(Q, dtype=float), (B, self.nq)), (B, self.nq))
        free, places = self._response_sets(keep_kinematic, constant_q_list, drive)
        nD = len(places)
        mu_in = None if mu is None else _lib.as_f64(np.broadcast_to(np.asarray(mu, dtype=float), (B, self.nc)), (B, self.nc))
        dq, dmu = np.zeros((B, nD, self.nq)), np.zeros((B, nD, self.nc))
        C = np.zeros((B, self.nq, self.nq)) if compliance else None
        R = np.zeros((B, self.nq, self.nc)) if compliance else None
        rank, status = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        mu_out, residual, defect = np.zeros((B, self.nc)), np.zeros(B), np.zeros(B)
        rc = self._L.tg_batch_static_response(self._h, _lib.ptr(Q), _lib.ptr(mu_in), free.ctypes.data, nD, places.ctypes.data, 1 if compliance else 0,
                                              float(rcond), dq.ctypes.data, dmu.ctypes.data, None if C is None else C.ctypes.data,
                                              None if R is None else R.ctypes.data, rank.ctypes.data, _lib.ptr(mu_out), residual.ctypes.data,
                                              defect.ctypes.data, status.ctypes.data)
        if rc == _lib.ERR_INVALID:
            raise ValueError(self._L.tg_last_error().decode())
        _lib.check(rc)
        return StaticResponse(dq, dmu, C, R, rank, mu_out, residual, defect, status)

    def static_response_device(self, Q_dev, mu_dev=None, keep_kinematic=False, constant_q_list=None, drive=None, compliance=True, rcond=1e-9,
                               dq_dev=None, dmu_dev=None, compliance_dev=None, reaction_dev=None, rank_dev=None, mu_out_dev=None,
                               residual_dev=None, defect_dev=None, status_dev=None):
        """static_response on device pointers, asynchronous on the batch's stream (tg_batch_static_response_device).  Q_dev
        [B][nq], mu_dev [B][nc] or None; the outputs are laid out as static_response returns them.  dq_dev and dmu_dev are needed
        where a config is driven, compliance_dev and reaction_dev with compliance=True; the others may be None.  The mask and the
        drive list stay host arguments.  Returns the number of driven configs."""
        self.refresh()
        free, places = self._response_sets(keep_kinematic, constant_q_list, drive)
        rc = self._L.tg_batch_static_response_device(self._h, Q_dev, mu_dev, free.ctypes.data, len(places), places.ctypes.data, 1 if compliance else 0,
                                                     float(rcond), dq_dev, dmu_dev, compliance_dev, reaction_dev, rank_dev, mu_out_dev, residual_dev,
                                                     defect_dev, status_dev)
        if rc == _lib.ERR_INVALID:
            raise ValueError(self._L.tg_last_error().decode())
        _lib.check(rc)
        return len(places)

    def _with_step_sizes(self, dts, call):
        """call() under the by-step list dts (None: as the batch stands); the list set before is put back."""
        if dts is None:
            return call()
        saved = getattr(self, "_step_sizes", None)
        self.set_step_sizes(dts)
        try:
            return call()
        finally:
            self.set_step_sizes(*(saved if saved is not None else (None,)))

    def inverse_dynamics(self, Q, dt, p0=None, ridge=0.0, rcond=None, bounds=None):
        """Inputs and constraint forces of given paths (include/trep_amd.h, tg_batch_inverse_dynamics): Q [B][N+1][nq], kinematic
        configs included; `dt` a scalar or one step size per step; p0 [B][nd], optional.  Every step (b, k) is one least-squares
        solve for the impulses (dt_k u_k, lambda_k), all B x N of them in one launch.  Returns the namedtuple (U [B][N][nu], lam
        [B][N][nc], P [B][N+1][nd], rho [B][N][nd], h [B][N][nc], status [B][N]): rho is the impulse no input can supply (zero on a
        feasible path), h = h(Q[k+1]), P[k+1] = D2L_d(Q[k], Q[k+1]) and P[0] = p0.  Without p0 step 0 is not solved: P[0] is the
        momentum that makes it force-free and U[0] = 0, so that initialize_from_state(t0, Q[:, 0], P[:, 0]) and rollout(N, dt, U, K)
        retrace Q (inverse_dynamics_trajectory packs that).  status: TG_OK, or TG_SINGULAR where the solver rejected the step (U,
        lam, rho zero there).  ridge >= 0 weighs |(dt u, lambda)|^2 against |rho|^2; it is required (ValueError) when nu + nc > nd,
        and a rank-deficient system needs it too -- that is not detected.  With a parameter table each trajectory uses its row.
        The integrator state of the batch is left alone.
        rcond (a float in [0, 1); None: the path above, unchanged) answers by rank-revealing least squares instead
        (tg_batch_inverse_dynamics_lsq): the impulses are numpy.linalg.lstsq's minimum-norm answer on [A~; sqrt(ridge) I], so a
        rank-deficient system needs no ridge and nu + nc > nd is accepted without one.  The namedtuple then has rank [B][N] as an
        additional last field (0 for a step that is not solved).
        bounds = (lo, hi) (None: the paths above, unchanged) confines (u | lambda) to a box, as in dynamics_inverse
        (tg_batch_inverse_dynamics_bounded): lo and hi are [nu + nc] or [B][nu + nc], a scalar broadcasts, None or +-inf mean no
        bound; rcond then defaults to 1e-9.  The bounds on u are FORCES, like the U returned (each step scales them by its own dt_k
        for the impulses it solves for); the bounds on lambda apply to lam as returned.  rho is then the impulse that inputs and
        constraints cannot supply WITHIN the box: a path that needs a string to push shows it there instead of in a negative
        tension.  The namedtuple has active [B][N][nu + nc] and solves [B][N] behind rank.  A string (Distance constraint) pulls where
        lambda >= 0 HERE (the integrator's sign): tension_bounds("inverse_dynamics")."""
        self.refresh()
        B = self._batch
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        if Q.ndim != 3 or Q.shape[0] != B or Q.shape[1] < 2 or Q.shape[2] != self.nq:
            raise ValueError("expected Q of shape (%d, N + 1, %d) with N >= 1, got %r" % (B, self.nq, Q.shape))
        N = Q.shape[1] - 1
        dt, dts = self._dt_argument(dt, N)
        p0 = None if p0 is None else _lib.as_f64(np.broadcast_to(np.asarray(p0, dtype=float), (B, self.nd)), (B, self.nd))
        U, lam, P = np.zeros((B, N, self.nu)), np.zeros((B, N, self.nc)), np.zeros((B, N + 1, self.nd))
        rho, h, status = np.zeros((B, N, self.nd)), np.zeros((B, N, self.nc)), np.zeros((B, N), dtype=np.int32)
        rank = np.zeros((B, N), dtype=np.int32)
        if bounds is not None:
            lo, hi, rows = self._box(bounds)
            active, solves = np.zeros((B, N, self.nu + self.nc), dtype=np.int32), np.zeros((B, N), dtype=np.int32)

        def call():
            p0_ptr = None if p0 is None else p0.ctypes.data
            if bounds is not None:
                rc = self._L.tg_batch_inverse_dynamics_bounded(self._h, N, dt, Q.ctypes.data, p0_ptr, float(ridge),
                                                               float(1e-9 if rcond is None else rcond), _lib.ptr(lo), _lib.ptr(hi), rows,
                                                               _lib.ptr(U), _lib.ptr(lam), _lib.ptr(P), _lib.ptr(rho), _lib.ptr(h),
                                                               _lib.ptr(active), solves.ctypes.data, rank.ctypes.data, status.ctypes.data)
            elif rcond is None:
                rc = self._L.tg_batch_inverse_dynamics(self._h, N, dt, Q.ctypes.data, p0_ptr, float(ridge), _lib.ptr(U), _lib.ptr(lam),
                                                       _lib.ptr(P), _lib.ptr(rho), _lib.ptr(h), status.ctypes.data)
            else:
                rc = self._L.tg_batch_inverse_dynamics_lsq(self._h, N, dt, Q.ctypes.data, p0_ptr, float(ridge), float(rcond), _lib.ptr(U),
                                                           _lib.ptr(lam), _lib.ptr(P), _lib.ptr(rho), _lib.ptr(h), rank.ctypes.data,
                                                           status.ctypes.data)
            if rc == _lib.ERR_INVALID:
                raise ValueError(self._L.tg_last_error().decode())
            _lib.check(rc)
        self._with_step_sizes(dts, call)
        if bounds is not None:
            return InverseDynamicsBounded(U, lam, P, rho, h, status, rank, active, solves)
        if rcond is None:
            return InverseDynamics(U, lam, P, rho, h, status)
        return InverseDynamicsRank(U, lam, P, rho, h, status, rank)

    def inverse_dynamics_device(self, n_steps, dt, Q_dev, q_row_stride=None, p0_dev=None, ridge=0.0, U_dev=None, lam_dev=None,
                                P_dev=None, rho_dev=None, h_dev=None, status_dev=None, rcond=None, rank_dev=None, bounds_dev=None,
                                active_dev=None, solves_dev=None):
        """inverse_dynamics on device pointers, asynchronous on the batch's stream (tg_batch_inverse_dynamics_device).  Row (b, k) of
        the path is read at Q_dev + (b (n_steps + 1) + k) q_row_stride doubles: the default nq for a packed Q, nX to read the
        configurations straight from a rollout's X [B][N+1][nX].  Any output may be None.  The step sizes are the scalar dt or the
        by-step list the batch has (set_step_sizes).  rcond (None: the path above): the rank-revealing path
        (tg_batch_inverse_dynamics_lsq_device), with rank_dev int32 [B][n_steps] or None.  bounds_dev = (lo_dev, hi_dev, rows): the
        bounded path (tg_batch_inverse_dynamics_bounded_device), as in dynamics_inverse_device; the u bounds are forces."""
        self.refresh()
        stride = int(self.nq if q_row_stride is None else q_row_stride)
        if bounds_dev is None and (active_dev is not None or solves_dev is not None):
            raise ValueError("active_dev and solves_dev need bounds_dev")
        if bounds_dev is not None:
            lo_dev, hi_dev, rows = bounds_dev
            rc = self._L.tg_batch_inverse_dynamics_bounded_device(self._h, int(n_steps), float(dt), Q_dev, stride, p0_dev, float(ridge),
                                                                  float(1e-9 if rcond is None else rcond), lo_dev, hi_dev, int(rows), U_dev,
                                                                  lam_dev, P_dev, rho_dev, h_dev, active_dev, solves_dev, rank_dev, status_dev)
        elif rcond is None:
            if rank_dev is not None:
                raise ValueError("rank_dev needs rcond")
            rc = self._L.tg_batch_inverse_dynamics_device(self._h, int(n_steps), float(dt), Q_dev, stride, p0_dev, float(ridge), U_dev, lam_dev,
                                                          P_dev, rho_dev, h_dev, status_dev)
        else:
            rc = self._L.tg_batch_inverse_dynamics_lsq_device(self._h, int(n_steps), float(dt), Q_dev, stride, p0_dev, float(ridge), float(rcond),
                                                              U_dev, lam_dev, P_dev, rho_dev, h_dev, rank_dev, status_dev)
        if rc == _lib.ERR_INVALID:
            raise ValueError(self._L.tg_last_error().decode())
        _lib.check(rc)

    def inverse_dynamics_trajectory(self, Q, dt, p0=None, ridge=0.0):
        """inverse_dynamics packed for rollout_closed_loop and discopt: returns (X [B][N+1][nX], U_full [B][N][nU], result) with
        X[k] = [Q[k]; P[k]; v[k]], v[k] = (Q[k][nd:] - Q[k-1][nd:]) / dt[k-1] (v[0] = 0: DSystem's state, dsystem.py:276-281) and
        U_full[k] = [U[k]; Q[k+1][nd:]] (its input: the forces and the kinematic configs' targets)."""
        r = self.inverse_dynamics(Q, dt, p0=p0, ridge=ridge)
        Q = np.asarray(Q, dtype=float)
        N = Q.shape[1] - 1
        dts = np.broadcast_to(np.asarray(dt, dtype=float).reshape(-1), (N,)) if np.ndim(dt) else np.full(N, float(dt))
        v = np.zeros((self._batch, N + 1, self.nk))
        v[:, 1:] = (Q[:, 1:, self.nd:] - Q[:, :-1, self.nd:]) / dts[None, :, None]
        X = np.concatenate([Q, r.P, v], axis=2)
        U_full = np.concatenate([r.U, Q[:, 1:, self.nd:]], axis=2)
        return X, U_full, r

    def _frame_indices(self, frames):
        """frames (Frame objects, names or indices into system.frames; None: all of them) -> contiguous int32 indices."""
        all_frames = self._system.frames
        if frames is None:
            return np.arange(len(all_frames), dtype=np.int32)
        place = {id(f): i for i, f in enumerate(all_frames)}
        out = []
        for f in frames:
            if isinstance(f, (int, np.integer)):
                if not 0 <= int(f) < len(all_frames):
                    raise ValueError("frame index %d outside the system's %d frames" % (int(f), len(all_frames)))
                out.append(int(f))
            else:
                out.append(place[id(self._system.get_frame(f))])
        if not out:
            raise ValueError("no frames selected")
        return np.array(out, dtype=np.int32)

    def frame_kinematics(self, Q, dQ=None, frames=None, jacobians=False):
        """Where the frames are (include/trep_amd.h, tg_batch_frame_kinematics): Q [B][nq] or [B][M][nq], kinematic configs included,
        dQ of the same shape or None; `frames` a list of Frame objects, names or indices into system.frames (default: all of them;
        repeats and any order allowed).  Every state is one team, all B x M of them in one launch.  Returns the namedtuple (g
        [B][M][F][3][4], vb [B][M][F][6], p_dq [B][M][F][nq][3], vb_ddq [B][M][F][nq][6]): rows 0..2 of Frame.g() (g[..., 3] is
        Frame.p()), Frame.vb() as (v, omega), Frame.p_dq(k)[:3] and Frame.vb_ddq(k) as (v, omega) for every config k (zero off the
        frame's path).  vb is None without dQ, the Jacobians are None without jacobians=True; for Q [B][nq] the M axis is dropped.
        Masses, parameters, a specialised library and the time base have no say; the integrator state of the batch is left alone."""
        self.refresh()
        B, nq = self._batch, self.nq
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        flat = Q.ndim == 2
        if flat:
            Q = Q[:, None, :]
        if Q.ndim != 3 or Q.shape[0] != B or Q.shape[1] < 1 or Q.shape[2] != nq:
            raise ValueError("expected Q of shape (%d, %d) or (%d, M, %d) with M >= 1, got %r" % (B, nq, B, nq, Q.shape))
        M = Q.shape[1]
        if dQ is not None:
            dQ = np.ascontiguousarray(dQ, dtype=np.float64)
            dQ = _lib.as_f64(dQ[:, None, :] if flat and dQ.ndim == 2 else dQ, (B, M, nq))
        idx = self._frame_indices(frames)
        F = len(idx)
        g = np.zeros((B, M, F, 3, 4))
        vb = None if dQ is None else np.zeros((B, M, F, 6))
        p_dq = np.zeros((B, M, F, nq, 3)) if jacobians else None
        vb_ddq = np.zeros((B, M, F, nq, 6)) if jacobians else None
        rc = self._L.tg_batch_frame_kinematics(self._h, M, Q.ctypes.data, None if dQ is None else dQ.ctypes.data, F, idx.ctypes.data,
                                               g.ctypes.data, None if vb is None else vb.ctypes.data,
                                               None if p_dq is None else p_dq.ctypes.data, None if vb_ddq is None else vb_ddq.ctypes.data)
        if rc == _lib.ERR_INVALID:
            raise ValueError(self._L.tg_last_error().decode())
        _lib.check(rc)
        drop = (lambda a: None if a is None else a[:, 0]) if flat else (lambda a: a)
        return FrameKinematics(drop(g), drop(vb), drop(p_dq), drop(vb_ddq))

    def frame_kinematics_device(self, n_states, Q_dev, q_row_stride=None, dQ_dev=None, dq_row_stride=None, frames=None, g_dev=None,
                                vb_dev=None, p_dq_dev=None, vb_ddq_dev=None):
        """frame_kinematics on device pointers, asynchronous on the batch's stream (tg_batch_frame_kinematics_device).  Row (b, m) is
        read at Q_dev + (b n_states + m) q_row_stride doubles (dQ_dev likewise with dq_row_stride): the default nq for packed
        arrays, nX to read the configurations straight from a rollout's X [B][n_states][nX].  The outputs are laid out as
        frame_kinematics returns them ([B][n_states][F]...); any may be None, not all.  `frames` as for frame_kinematics; while it
        stays the same from call to call nothing is allocated."""
        self.refresh()
        idx = self._frame_indices(frames)
        rc = self._L.tg_batch_frame_kinematics_device(self._h, int(n_states), Q_dev, int(self.nq if q_row_stride is None else q_row_stride),
                                                      dQ_dev, int(self.nq if dq_row_stride is None else dq_row_stride), len(idx),
                                                      idx.ctypes.data, g_dev, vb_dev, p_dq_dev, vb_ddq_dev)
        if rc == _lib.ERR_INVALID:
            raise ValueError(self._L.tg_last_error().decode())
        _lib.check(rc)

    def _measure_tables(self, measures):
        """measures (each a TapeMeasure of this system or a sequence of frames by name, object or index) -> (start [T + 1], frames)
        as contiguous int32, the layout of tg_batch_tape_measures.  Raises ValueError for what the library would refuse."""
        from .tapemeasure import TapeMeasure
        if measures is None or isinstance(measures, (TapeMeasure, str)) or len(measures) == 0:
            raise ValueError("measures: a non-empty list of TapeMeasure objects or frame sequences")
        start, flat = [0], []
        for m in measures:
            if isinstance(m, TapeMeasure):
                if m.system is not self._system:
                    raise ValueError("a TapeMeasure of another system")
                m = m.frames
            elif isinstance(m, str):
                raise ValueError("a measure is a sequence of frames, not one name")
            try:
                idx = [] if len(m) == 0 else [int(i) for i in self._frame_indices(m)]
            except (KeyError, TypeError) as e:          # an unknown name, a frame of another system, not a frame at all
                raise ValueError("not a frame of this system in a measure: %s" % (e,))
            if len(idx) < 2:
                raise ValueError("a measure needs at least two frames")
            if any(a == b for a, b in zip(idx[:-1], idx[1:])):
                raise ValueError("two equal consecutive frames in a measure")
            flat += idx
            start.append(len(flat))
        return np.array(start, dtype=np.int32), np.array(flat, dtype=np.int32)

    def tape_measures(self, Q, dQ=None, measures=None, gradients=False, hessians=False):
        """Lengths of broken lines through frame origins (include/trep_amd.h, tg_batch_tape_measures): Q [B][nq] or [B][M][nq], kinematic
        configs included, dQ of the same shape or None; `measures` a list whose items are trep_amd.TapeMeasure objects of this system
        or sequences of frames (names, Frame objects or indices into system.frames; at least two, consecutive ones different).  Every
        state is one team, all B x M of them in one launch.  Returns the namedtuple (length [B][M][T], velocity [B][M][T], length_dq
        [B][M][T][nq], velocity_dq [B][M][T][nq], length_dqdq [B][M][T][nq][nq]): what TapeMeasure.length(), velocity(), length_dq(k)
        (= velocity_ddq(k)), velocity_dq(k) and length_dqdq(j, k) (= velocity_ddqdq(j, k)) return at each state.  velocity and
        velocity_dq are None without dQ, the two gradients without gradients=True, the Hessian without hessians=True; for Q [B][nq]
        the M axis is dropped.  A config that moves no segment of a measure has exact zeros there.  A segment of zero length gives
        non-finite values for its measure, as on the host.  The integrator state of the batch is left alone."""
        self.refresh()
        B, nq = self._batch, self.nq
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        flat = Q.ndim == 2
        if flat:
            Q = Q[:, None, :]
        if Q.ndim != 3 or Q.shape[0] != B or Q.shape[1] < 1 or Q.shape[2] != nq:
            raise ValueError("expected Q of shape (%d, %d) or (%d, M, %d) with M >= 1, got %r" % (B, nq, B, nq, Q.shape))
        M = Q.shape[1]
        if dQ is not None:
            dQ = np.ascontiguousarray(dQ, dtype=np.float64)
            dQ = _lib.as_f64(dQ[:, None, :] if flat and dQ.ndim == 2 else dQ, (B, M, nq))
        start, frames = self._measure_tables(measures)
        T = len(start) - 1
        length = np.zeros((B, M, T))
        velocity = None if dQ is None else np.zeros((B, M, T))
        length_dq = np.zeros((B, M, T, nq)) if gradients else None
        velocity_dq = np.zeros((B, M, T, nq)) if gradients and dQ is not None else None
        length_dqdq = np.zeros((B, M, T, nq, nq)) if hessians else None
        ptr = lambda a: None if a is None else a.ctypes.data
        rc = self._L.tg_batch_tape_measures(self._h, M, Q.ctypes.data, ptr(dQ), T, start.ctypes.data, frames.ctypes.data, ptr(length),
                                            ptr(velocity), ptr(length_dq), ptr(velocity_dq), ptr(length_dqdq))
        if rc == _lib.ERR_INVALID:
            raise ValueError(self._L.tg_last_error().decode())
        _lib.check(rc)
        drop = (lambda a: None if a is None else a[:, 0]) if flat else (lambda a: a)
        return TapeMeasures(drop(length), drop(velocity), drop(length_dq), drop(velocity_dq), drop(length_dqdq))

    def tape_measures_device(self, n_states, Q_dev, q_row_stride=None, dQ_dev=None, dq_row_stride=None, measures=None, length_dev=None,
                             velocity_dev=None, length_dq_dev=None, velocity_dq_dev=None, length_dqdq_dev=None):
        """tape_measures on device pointers, asynchronous on the batch's stream (tg_batch_tape_measures_device).  Row (b, m) is read at
        Q_dev + (b n_states + m) q_row_stride doubles (dQ_dev likewise with dq_row_stride): the default nq for packed arrays, nX to
        read the configurations straight from a rollout's X [B][n_states][nX].  The outputs are laid out as tape_measures returns them ([B][n_states][T]...); any may be None, not all; the two
        velocity outputs need dQ_dev.  `measures` as for tape_measures; while it stays the same from call to call nothing is allocated."""
        self.refresh()
        start, frames = self._measure_tables(measures)
        rc = self._L.tg_batch_tape_measures_device(self._h, int(n_states), Q_dev, int(self.nq if q_row_stride is None else q_row_stride),
                                                   dQ_dev, int(self.nq if dq_row_stride is None else dq_row_stride), len(start) - 1,
                                                   start.ctypes.data, frames.ctypes.data, length_dev, velocity_dev, length_dq_dev,
                                                   velocity_dq_dev, length_dqdq_dev)
        if rc == _lib.ERR_INVALID:
            raise ValueError(self._L.tg_last_error().decode())
        _lib.check(rc)

    def _seeds(self, seeds, most):
        """(seed1,) or (seed1, seed2) -> contiguous int32 [B] arrays: the input variable each trajectory's direction follows, numbered
        q [nq] | dq [nq] | ddq_k [nk] | u [nu] (forward-mode kernels, csrc/dual.hpp)."""
        if not 1 <= len(seeds) <= most:
            raise ValueError("between one and %d direction arrays" % most)
        out = [np.ascontiguousarray(np.broadcast_to(np.asarray(s_, dtype=np.int32), (self._batch,))) for s_ in seeds]
        return out

    def lagrangian(self, Q, dQ, seeds=None):
        """First and second derivatives of the Lagrangian of B states: dict with L_dq, L_ddq [B][nq] and L_dqdq,
        L_ddqdq (velocity config = row), L_ddqddq [B][nq][nq] (System.L_dq() ... L_ddqddq(), system.py:852-925).
        seeds = (s1,) or (s1, s2): the exact derivative of every entry along input variable s1[b] (and s2[b]) instead --
        the third- and fourth-order derivatives System.L_dqdqdq() ... L_ddqddqdqdq() (system.py:869-949)."""
        self.refresh()
        B = self._batch
        Q = _lib.as_f64(np.broadcast_to(np.asarray(Q, dtype=float), (B, self.nq)), (B, self.nq))
        dQ = _lib.as_f64(np.broadcast_to(np.asarray(dQ, dtype=float), (B, self.nq)), (B, self.nq))
        o1, o2 = np.zeros((B, 2, self.nq)), np.zeros((B, 3, self.nq, self.nq))
        if seeds is None:
            _lib.check(self._L.tg_batch_lagrangian(self._h, _lib.ptr(Q), _lib.ptr(dQ), _lib.ptr(o1), _lib.ptr(o2)))
        else:
            sd = self._seeds(seeds, 2)
            _lib.check(self._L.tg_batch_lagrangian_forward(self._h, _lib.ptr(Q), _lib.ptr(dQ), sd[0].ctypes.data,
                                                           sd[1].ctypes.data if len(sd) > 1 else None, _lib.ptr(o1), _lib.ptr(o2)))
        return {"L_dq": o1[:, 0], "L_ddq": o1[:, 1], "L_dqdq": o2[:, 0], "L_ddqdq": o2[:, 1], "L_ddqddq": o2[:, 2]}

    @property
    def predictor(self):
        """Initial guess of the rollouts' Newton iteration: "reference" (q2 <- previous q2, the reference's semantics
        and iteration counts) or "extrapolate" (q2 + (q2 - q1) dt_k / dt_{k-1}: same trajectory to solver tolerance, fewer iterations)."""
        return getattr(self, "_predictor", "reference")

    @predictor.setter
    def predictor(self, mode):
        modes = {"reference": 0, "extrapolate": 1}
        if mode not in modes:
            raise ValueError("predictor must be one of %r" % sorted(modes))
        _lib.check(self._L.tg_batch_set_predictor(self._h, modes[mode]))
        self._predictor = mode

    def energy(self, Q, dQ):
        """Kinetic and potential energy of B states: [B][2] = (T, V); the reference's System.L() is T - V and
        System.total_energy() T + V (system.py:844-850)."""
        self.refresh()
        B = self._batch
        Q = _lib.as_f64(np.broadcast_to(np.asarray(Q, dtype=float), (B, self.nq)), (B, self.nq))
        dQ = _lib.as_f64(np.broadcast_to(np.asarray(dQ, dtype=float), (B, self.nq)), (B, self.nq))
        out = np.zeros((B, 2))
        _lib.check(self._L.tg_batch_energy(self._h, _lib.ptr(Q), _lib.ptr(dQ), _lib.ptr(out)))
        return out

    DYN_D1_NAMES = ("f_dq", "f_ddq", "f_dddk", "f_du", "lambda_dq", "lambda_ddq", "lambda_dddk", "lambda_du")

    def dynamics_deriv1(self, Q, dQ, U=None, ddQk=None, seeds=None):
        """First derivatives of the continuous dynamics of B states at once (System.f_dq() ... lambda_du() of the
        reference, system.py:961-1044).  Returns ({name: [B][output][derivative variable]}, status [B]).
        seeds = (s,): the exact derivative of every entry along input variable s[b] instead (the first-derivative kernel on dual
        numbers): the second derivatives System.f_dqdq() ... lambda_dudu() (system.py:982-1078), one variable per trajectory."""
        self.refresh()
        B = self._batch
        Q = _lib.as_f64(np.broadcast_to(np.asarray(Q, dtype=float), (B, self.nq)), (B, self.nq))
        dQ = _lib.as_f64(np.broadcast_to(np.asarray(dQ, dtype=float), (B, self.nq)), (B, self.nq))
        U = np.zeros((B, self.nu)) if U is None else _lib.as_f64(np.broadcast_to(np.asarray(U, dtype=float), (B, self.nu)), (B, self.nu))
        K = np.zeros((B, self.nk)) if ddQk is None else _lib.as_f64(np.broadcast_to(np.asarray(ddQk, dtype=float), (B, self.nk)), (B, self.nk))
        rows = (self.nq, self.nq, self.nk, self.nu)
        outs = [np.zeros((B, rows[g & 3], self.nd if g < 4 else self.nc)) for g in range(8)]
        status = np.zeros(B, dtype=np.int32)
        if seeds is None:
            _lib.check(self._L.tg_batch_dynamics_deriv1(self._h, _lib.ptr(Q), _lib.ptr(dQ), _lib.ptr(U), _lib.ptr(K),
                                                        *([_lib.ptr(o) for o in outs] + [status.ctypes.data])))
        else:
            sd = self._seeds(seeds, 1)
            _lib.check(self._L.tg_batch_dynamics_deriv1_forward(self._h, _lib.ptr(Q), _lib.ptr(dQ), _lib.ptr(U), _lib.ptr(K), sd[0].ctypes.data,
                                                                *([_lib.ptr(o) for o in outs] + [status.ctypes.data])))
        return dict((n, np.swapaxes(o, 1, 2)) for n, o in zip(self.DYN_D1_NAMES, outs)), status

    def snapshot(self):
        """Save the integrator state on the device (replayed by restore())."""
        _lib.check(self._L.tg_batch_snapshot(self._h))

    def restore(self):
        _lib.check(self._L.tg_batch_restore(self._h))

    def status(self):
        iters = np.zeros(self._batch, dtype=np.int32)
        status = np.zeros(self._batch, dtype=np.int32)
        _lib.check(self._L.tg_batch_status(self._h, iters.ctypes.data, status.ctypes.data))
        return iters, status

    def solver_fallbacks(self):
        """Per trajectory: Newton systems of the last rollout / step launch that the structured solve of the specialised kernel handed
        to the pivoting solver (a failed pivot guard; results are unaffected).  tg_batch_solver_fallbacks."""
        out = np.zeros(self.batch, dtype=np.int32)
        _lib.check(self._L.tg_batch_solver_fallbacks(self._h, out.ctypes.data_as(_lib._c_ip)))
        return out

    def synchronize(self):
        _lib.check(self._L.tg_batch_synchronize(self._h))

    def set_stream(self, hip_stream):
        _lib.check(self._L.tg_batch_set_stream(self._h, hip_stream))

    def timing(self, reset=True):
        """(number of kernel launches, summed HIP-event duration in ms) since the last reset."""
        import ctypes
        n = ctypes.c_int32()
        ms = ctypes.c_double()
        _lib.check(self._L.tg_batch_timing(self._h, 1 if reset else 0, ctypes.byref(n), ctypes.byref(ms)))
        return n.value, ms.value


class MidpointVI(object):
    """Drop-in for ``trep.MidpointVI`` (one trajectory) on top of a batch of one."""

    def __init__(self, system, tolerance=1e-10, num_threads=None, device=0, specialize="auto"):
        # num_threads: accepted and ignored (the reference's pthread pool, midpointvi.c:9-293,
        # is replaced by GPU parallelism).  specialize: as in BatchMidpointVI (not a reference argument).
        self._system = system
        self._device = device
        self._tolerance = tolerance
        self._specialize = specialize
        self._b = None
        self._cache = 0
        self._rebuild()
        system.add_structure_changed_func(self._structure_updated)

    def _structure_updated(self):
        self._stale = True

    def _rebuild(self):
        if self._b is not None:
            self._b.close()
        self._b = BatchMidpointVI(self._system, 1, self._tolerance, self._device, specialize=self._specialize)
        self._stale = False

    def _batch(self):
        if self._stale:
            # BatchMidpointVI.refresh() rebuilds the device schedule and, when the sizes are unchanged (a parameter
            # write such as `gravity.gravity = ...`), carries t, q, p, u, lambda over like the reference does
            if self._b.refresh():
                self._cache = 0
            self._stale = False
        return self._b

    def __repr__(self):
        return "<MidpointVI t1=%f t2=%f nd=%d nk=%d nc=%d nu=%d>" % (self.t1, self.t2, self.nd, self.nk, self.nc, self.nu)

    system = property(lambda self: self._system)
    nq = property(lambda self: self._batch().nq)
    nd = property(lambda self: self._batch().nd)
    nk = property(lambda self: self._batch().nk)
    nu = property(lambda self: self._batch().nu)
    nc = property(lambda self: self._batch().nc)

    @property
    def tolerance(self):
        return self._tolerance

    @tolerance.setter
    def tolerance(self, value):
        self._tolerance = value
        self._batch().tolerance = value

    def _vec(name):
        def getter(self):
            return getattr(self._batch(), name)[0].copy()

        def setter(self, value):
            self._cache = 0
            setattr(self._batch(), name, np.asarray(value, dtype=float)[None, :])
        return property(getter, setter)

    q1 = _vec("q1")
    q2 = _vec("q2")
    p1 = _vec("p1")
    p2 = _vec("p2")
    u1 = _vec("u1")
    lambda1 = _vec("lambda1")
    del _vec

    @property
    def t1(self):
        return self._batch().times()[0]

    @t1.setter
    def t1(self, t):
        self._cache = 0
        self._batch().set_times(t, self.t2)

    @property
    def t2(self):
        return self._batch().times()[1]

    @t2.setter
    def t2(self, t):
        self._cache = 0
        self._batch().set_times(self.t1, t)

    @property
    def v2(self):
        """Discrete kinematic velocity (q2k - q1k)/(t2 - t1) (midpointvi.py:325-332)."""
        t1, t2 = self._batch().times()
        if t2 != t1:
            return ((self.q2 - self.q1) / (t2 - t1))[self.nd:]
        return None

    # -- derivative accessors (midpointvi.py:337-371, 474-506, 604-640): Config / Input / Constraint
    #    objects or None (= whole axis) select entries; the result is output-major like the reference.
    def _calc_deriv1(self):
        if self._cache & 2:
            return
        if not (self._cache & 1):
            raise Exception("Integrator has not solved of the next time step yet.")
        b = self._batch()
        b.calc_deriv1()
        self._d1 = dict((n, b.deriv1(n)[0]) for n in b.D1_NAMES)
        self._cache |= 2

    def deriv2_contract(self, z):
        """HZ [R][R] for one contraction vector z (nX); see BatchMidpointVI.deriv2_contract."""
        if not (self._cache & 1):
            raise Exception("Integrator has not solved of the next time step yet.")
        return self._batch().deriv2_contract(np.asarray(z, dtype=float)[None, :])[0]

    # -- full second-derivative tensors (midpointvi.py:373-469, 508-600): assembled from 2*nd unit-vector
    #    contractions run as ONE batched launch on a helper batch holding copies of the solved step.
    def _calc_deriv2(self):
        if self._cache & 4:
            return
        if not (self._cache & 1):
            raise Exception("Integrator has not solved of the next time step yet.")
        b = self._batch()
        nd, nq, nu, nk = b.nd, b.nq, b.nu, b.nk
        nc = b.nc
        if getattr(self, "_b2", None) is None or self._b2_version != self._system._structure_version:
            self._b2 = BatchMidpointVI(self._system, max(2 * nd + nc, 1), self._tolerance, self._device, specialize=self._specialize)
            self._b2_version = self._system._structure_version
        h = self._b2
        h.set_times(*b.times())
        for name in ("q1", "q2", "p1", "p2", "u1", "lambda1"):
            setattr(h, name, getattr(b, name)[0])
        # one unit contraction per output: nd for q2, nd for p2, nc for lambda1
        Z = np.zeros((2 * nd + nc, b.nX))
        ZL = np.zeros((2 * nd + nc, nc))
        Z[np.arange(nd), np.arange(nd)] = 1.0
        Z[nd + np.arange(nd), nq + np.arange(nd)] = 1.0
        ZL[2 * nd + np.arange(nc), np.arange(nc)] = 1.0
        HZ = h.deriv2_contract(Z, ZL if nc else None)
        off = {"dq1": (0, nq), "dp1": (nq, nd), "du1": (nq + nd, nu), "dk2": (nq + nd + nu, nk)}
        self._d2 = {}
        names = ["dq1", "dp1", "du1", "dk2"]
        for ia, a in enumerate(names):
            for bname in names[ia:]:
                (oa, na), (ob, nb) = off[a], off[bname]
                blk = HZ[:, oa:oa + na, ob:ob + nb]
                self._d2["q2_" + a + bname] = np.ascontiguousarray(np.moveaxis(blk[:nd], 0, 2))
                self._d2["p2_" + a + bname] = np.ascontiguousarray(np.moveaxis(blk[nd:2 * nd], 0, 2))
                self._d2["lambda1_" + a + bname] = np.ascontiguousarray(np.moveaxis(blk[2 * nd:], 0, 2))
        self._cache |= 4

    def _d2_accessor(name, kinds):
        def accessor(self, out=None, var1=None, var2=None):
            self._calc_deriv2()
            out_kind = "c" if name.startswith("lambda1") else "d"
            return self._d2[name][self._index(var1, kinds[0]), self._index(var2, kinds[1]), self._index(out, out_kind)].copy()
        accessor.__name__ = name
        return accessor

    for _pre in ("q2", "p2", "lambda1"):
        for _pair, _kinds in (("dq1dq1", "qq"), ("dq1dp1", "qd"), ("dq1du1", "qu"), ("dq1dk2", "qk"), ("dp1dp1", "dd"),
                              ("dp1du1", "du"), ("dp1dk2", "dk"), ("du1du1", "uu"), ("du1dk2", "uk"), ("dk2dk2", "kk")):
            locals()["%s_%s" % (_pre, _pair)] = _d2_accessor("%s_%s" % (_pre, _pair), _kinds)
    del _d2_accessor, _pre, _pair, _kinds

    @staticmethod
    def _index(obj, kind):
        if obj is None:
            return slice(None)
        if kind == "k":
            assert obj.kinematic
            return obj.k_index
        if kind == "d":
            assert not obj.kinematic
        return obj.index

    def _d1_accessor(name, out_kind, var_kind):
        def accessor(self, out=None, var=None):
            self._calc_deriv1()
            return self._d1[name][self._index(var, var_kind), self._index(out, out_kind)].T.copy()
        accessor.__name__ = name
        return accessor

    q2_dq1 = _d1_accessor("q2_dq1", "d", "q")
    q2_dp1 = _d1_accessor("q2_dp1", "d", "d")
    q2_du1 = _d1_accessor("q2_du1", "d", "u")
    q2_dk2 = _d1_accessor("q2_dk2", "d", "k")
    p2_dq1 = _d1_accessor("p2_dq1", "d", "q")
    p2_dp1 = _d1_accessor("p2_dp1", "d", "d")
    p2_du1 = _d1_accessor("p2_du1", "d", "u")
    p2_dk2 = _d1_accessor("p2_dk2", "d", "k")
    lambda1_dq1 = _d1_accessor("l1_dq1", "c", "q")
    lambda1_dp1 = _d1_accessor("l1_dp1", "c", "d")
    lambda1_du1 = _d1_accessor("l1_du1", "c", "u")
    lambda1_dk2 = _d1_accessor("l1_dk2", "c", "k")
    del _d1_accessor

    def initialize_from_state(self, t1, q1, p1, lambda1=None):
        self._cache = 0
        self._batch().initialize_from_state(t1, np.asarray(q1, dtype=float)[None, :], np.asarray(p1, dtype=float)[None, :],
                                            None if lambda1 is None else np.asarray(lambda1, dtype=float)[None, :])

    def initialize_from_configs(self, t0, q0, t1, q1, lambda1=None):
        self._cache = 0
        self._batch().initialize_from_configs(t0, np.asarray(q0, dtype=float)[None, :], t1, np.asarray(q1, dtype=float)[None, :],
                                              None if lambda1 is None else np.asarray(lambda1, dtype=float)[None, :])

    def calc_p2(self):
        self._batch().calc_p2()

    def calc_f(self):
        return self._batch().calc_f()[0]

    def set_midpoint(self):
        """Put the System object at the midpoint of the current step: q = (q1 + q2) / 2, dq = (q2 - q1) / (t2 - t1), u = u1,
        t = (t1 + t2) / 2 (midpointvi.c:430-455).  Host-side state of the model object only; the device state is untouched."""
        sys_ = self._system
        sys_.t = 0.5 * (self.t1 + self.t2)
        sys_.q = 0.5 * (np.asarray(self.q1) + np.asarray(self.q2))
        sys_.dq = (np.asarray(self.q2) - np.asarray(self.q1)) / (self.t2 - self.t1)
        if self.nu:
            sys_.u = self.u1

    def discrete_fm2(self):
        """The discrete forcing of the step, fm2_i = (t2 - t1) sum_forces f(q_i) at the midpoint state, for every dynamic
        config (midpointvi.c:478-482, 2710-2728).  Evaluated through the host-side force queries (Force.f)."""
        self.set_midpoint()
        dt = self.t2 - self.t1
        return np.array([dt * sum(f.f(q) for f in self._system.forces) for q in self._system.dyn_configs])

    def step(self, t2, u1=tuple(), k2=tuple(), max_iterations=200, q2_hint=None, lambda1_hint=None):
        """Advance to t2; returns the Newton iteration count, raises ConvergenceError like the
        reference (midpointvi.py:174-201; midpointvi.c:715-718; singular -> :198-201)."""
        u1 = np.array(u1, dtype=float)
        k2 = np.array(k2, dtype=float)
        assert u1.shape == (self.nu,)
        assert k2.shape == (self.nk,)
        self._cache = 0     # the reference's setters zero the cache before the solve (midpointvi.py:188-197, 250-323)
        iters, status = self._batch().step(t2, u1[None, :], k2[None, :], max_iterations, q2_hint, lambda1_hint)
        if status[0] == _lib.NOT_CONVERGED:
            raise ConvergenceError("failed to converge after %d iterations" % (max_iterations + 1))
        if status[0] == _lib.SINGULAR:
            raise ConvergenceError("Singular derivative of DEL at t=%s" % t2)
        self._cache = 1
        return int(iters[0])
