"""What every tg_batch_* / tg_system_* call answers to null handles and zero scalars: the return value and the tg_last_error() text.
No device is needed: the library refuses before it touches one.  The table was recorded from the library before its host layer
was rewritten around owned device buffers, and pins the first refusal of every entry point."""
import ctypes

import pytest

from trep_amd import _lib

# entry -> (return value, tg_last_error() text; None: the call sets no message)
REFUSALS = {
    "tg_system_sizes": (-1, "null system"),
    "tg_system_info": (-1, "null system"),
    "tg_batch_set_tolerance": (-1, "null batch"),
    "tg_batch_set_times": (-1, "null batch"),
    "tg_batch_get_times": (-1, "null batch"),
    "tg_batch_set": (-1, "null batch"),
    "tg_batch_get": (-1, "null batch"),
    "tg_batch_field_width": (-1, None),
    "tg_batch_calc_p2": (-1, "null batch"),
    "tg_batch_calc_f": (-1, "null argument"),
    "tg_batch_step": (-1, "null batch"),
    "tg_batch_rollout": (-1, "bad arguments"),
    "tg_batch_rollout_closed_loop": (-1, "bad arguments"),
    "tg_batch_rollout_stats": (-1, "null batch"),
    "tg_batch_status": (-1, "null batch"),
    "tg_batch_solver_fallbacks": (-1, "null argument"),
    "tg_batch_deriv1": (-1, "null batch"),
    "tg_batch_deriv2_contract": (-1, "null argument"),
    "tg_batch_dynamics": (-1, "null argument"),
    "tg_batch_dynamics_device": (-1, "null argument"),
    "tg_batch_dynamics_deriv1": (-1, "null argument"),
    "tg_batch_dynamics_deriv1_device": (-1, "null argument"),
    "tg_batch_energy": (-1, "null argument"),
    "tg_batch_lagrangian": (-1, "null argument"),
    "tg_batch_lagrangian_forward": (-1, "null argument"),
    "tg_batch_dynamics_deriv1_forward": (-1, "null argument"),
    "tg_batch_set_predictor": (-1, "predictor mode must be 0 or 1"),
    "tg_batch_deriv2_contract_lambda": (-1, "null argument"),
    "tg_batch_snapshot": (-1, "null batch"),
    "tg_batch_restore": (-1, "null batch"),
    "tg_batch_synchronize": (-1, "null batch"),
    "tg_batch_set_stream": (-1, "null batch"),
    "tg_batch_timing": (-1, "null batch"),
    "tg_system_newton_plan": (-1, "null argument"),
    "tg_batch_debug_newton_solve": (-1, "bad arguments"),
    "tg_batch_set_pivot_rule": (-1, "null batch"),
    "tg_batch_set_step_sizes": (-1, "bad arguments"),
    "tg_system_spec_header": (-1, "null system"),
    "tg_system_spec_key": (0, "null system"),
    "tg_batch_load_specialized": (-1, "null argument"),
    "tg_batch_info": (-1, "null argument"),
    "tg_system_parameters": (-1, "null system"),
    "tg_batch_set_parameters": (-1, "null batch"),
    "tg_batch_clear_parameters": (-1, "null batch"),
    "tg_batch_par_info": (-1, "null argument"),
    "tg_batch_stream": (None, None),
    "tg_batch_set_from_trajectories": (-1, "bad arguments"),
    "tg_batch_linearize": (-1, "null argument"),
    "tg_batch_initialize_from_state_device": (-1, "bad arguments"),
    "tg_batch_deriv2_contract_device": (-1, "null argument"),
    "tg_batch_deriv2_contract_device_range": (-1, "null argument"),
    "tg_batch_rollout_closed_loop_subset": (-1, "bad arguments"),
}
LIFETIME = {"tg_batch_create", "tg_batch_destroy", "tg_system_create", "tg_system_destroy"}
_SCALARS = {ctypes.c_double: 0.0, ctypes.c_int32: 0, ctypes.c_int: 0, ctypes.c_uint64: 0, ctypes.c_int64: 0}


def _mark(L):
    """A message no entry of the table gives: a call that leaves it in place has set none."""
    assert not L.tg_system_create(None)
    assert L.tg_last_error() == b"null descriptor"


def test_the_table_covers_the_abi():
    names = set(n for n in _lib._SIGNATURES if n.startswith(("tg_batch_", "tg_system_"))) - LIFETIME
    assert names == set(REFUSALS)


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_null_handles_and_zero_scalars_are_refused(name):
    L = _lib.lib()
    want, message = REFUSALS[name]
    args = [_SCALARS.get(t) for t in _lib._SIGNATURES[name][1]]       # pointers of every kind: None
    _mark(L)
    assert getattr(L, name)(*args) == want
    assert L.tg_last_error().decode() == ("null descriptor" if message is None else message)


def test_batch_create_refuses_a_null_system():
    L = _lib.lib()
    _mark(L)
    assert L.tg_batch_create(None, 0, 0) is None
    assert L.tg_last_error() == b"bad arguments"
