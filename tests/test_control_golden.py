"""The baseline controller, CPU-only checks (no kernel launches).

* the numpy controller oracle (tests/control_oracle.py) replays every fixture the reference's own
  control() produced (tests/golden/control, gen_golden_control.py) bit for bit -- which makes it
  a valid checker for the HIP kernels (tests/test_gpu_control.py);
* the library's host-side controller constant equals the fixtures';
* the new entry points fail on a NULL handle before they touch a device.
"""
import numpy as np
import pytest

import control_oracle as co
from oracle import NumpyOracleEnv

CASES = co.case_names()
WANT = ["f11_n12_d8", "f13_n10_d8", "f1_n1024_d8", "f2_n100_d8", "f2_n64_d8", "f2_n66_d6",
        "f3_n2_d8", "f7_n4_d6"]


def test_fixture_set_complete():
    assert CASES == WANT


@pytest.mark.parametrize("name", WANT)
def test_numpy_controller_replays_fixture(name):
    c = co.load_case(name)
    env = NumpyOracleEnv(c["F"], c["N"], c["goal_in_obs"], c["seed"])  # draw set 1
    env.reset()                                                        # draw set 2
    px, py, gx, gy, t = env.get_state()
    ag, gl = co.state_vec(px, py, gx, gy)
    assert np.array_equal(np.concatenate([ag, gl]).view(np.uint32),
                          c["state_reset"].view(np.uint32)), "reset state"
    for k in range(1, c["steps"] + 1):
        vel, obs, rew, done = co.control_step(env)
        co.check_step(c, k, vel, obs, rew, done, *env.get_state())


@pytest.mark.parametrize("name", WANT)
def test_control_neighbor_dist_matches_fixture(flib, name):
    c = co.load_case(name)
    got = np.float32(flib.lib().fenv_control_neighbor_dist(c["N"]))
    assert got.view(np.uint32) == c["dd"].view(np.uint32)
    assert got == co.control_neighbor_dist(c["N"])


def test_null_handle_rejected_without_device(flib):
    L = flib.lib()
    assert L.fenv_control(None, None, None) == -1
    assert b"fenv_control: NULL handle" in L.fenv_last_error()
    assert L.fenv_rollout_velocity(None, 1, None, None, None, None, None, None) == -1
    assert b"fenv_rollout_velocity: NULL handle" in L.fenv_last_error()
    assert L.fenv_rollout_control(None, 1, None, None, None, None, None, None) == -1
    assert b"fenv_rollout_control: NULL handle" in L.fenv_last_error()
