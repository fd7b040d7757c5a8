"""Numpy restatement of the reference's baseline controller -- TEST INFRASTRUCTURE ONLY.

``control(i, env)`` of the reference (simulate.py:256-319) over the state of a
:class:`oracle.NumpyOracleEnv`, in the reference's fp32 operation order, pinned bit for bit to
the reference itself by the fixtures under tests/golden/control (gen_golden_control.py), which
the HIP kernels (csrc/control_kernels.hip) are then held to.

Stepping with a velocity needs no copy of the oracle's step: the velocity is added to the
positions, then the oracle steps with zero actions, so its out-of-bounds test and clip act on
p + v exactly as the reference's do (simulate.py:82-90).
"""
from __future__ import annotations

import glob
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CONTROL_GOLDEN = os.path.join(HERE, "golden", "control")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from oracle import NumpyOracleEnv, norm2  # noqa: E402

from golden_util import d64  # noqa: E402

F32 = np.float32


def control_neighbor_dist(n: int) -> np.float32:
    """simulate.py:286 with desired_radius = 40 (:259): float64, rounded once to fp32."""
    return F32(np.pi * 40 / n)


def _clip1(v: np.ndarray) -> np.ndarray:
    """torch.clip(v, -1, 1); NaN propagates."""
    return np.where(v < F32(-1), F32(-1), np.where(v > F32(1), F32(1), v)).astype(F32)


def control_velocity(p: np.ndarray, g: np.ndarray) -> np.ndarray:
    """The velocity control() hands to env.step: p [F, N, 2] positions, g [F, 2] goals ->
    [F, N, 2], all float32.  N must be even (simulate.py:279)."""
    p = np.asarray(p, F32)
    g = np.asarray(g, F32)
    N = p.shape[1]
    assert N % 2 == 0
    dd = control_neighbor_dist(N)

    def term(q, des):
        d = norm2(p[..., 0] - q[..., 0], p[..., 1] - q[..., 1])[..., None]  # :270
        direction = ((q - p) / d).astype(F32)                               # :271-272
        return ((F32(0.02) * (d - des)).astype(F32) * direction).astype(F32)  # :290

    with np.errstate(invalid="ignore", divide="ignore"):
        nxt = np.roll(p, -1, axis=1)       # agents_shiftA (:262-264)
        prv = np.roll(p, 1, axis=1)        # agents_shiftB (:265-267)
        opp = np.roll(p, -(N // 2), axis=1)  # agents_opposite (:278-281)
        ff = ((term(nxt, dd) + term(prv, dd)).astype(F32) + term(opp, F32(80))).astype(F32)
        ff = _clip1(ff)                                                     # :293
        gd = (p - g[:, None, :]).astype(F32)                                # :311
        d = norm2(gd[..., 0], gd[..., 1])[..., None]                        # :312
        gdir = (gd / d).astype(F32)                                         # :313
        fg = _clip1(((-(F32(0.01) * (d - F32(40)))).astype(F32) * gdir).astype(F32))  # :315-317
        return ((ff + F32(0.0)).astype(F32) + fg).astype(F32)               # :319


def step_velocity(env: NumpyOracleEnv, v: np.ndarray):
    """FormationSimulator.step(v) of every formation of the oracle env (see the module text)."""
    env.p = (env.p + np.asarray(v, F32).reshape(env.F, env.N, 2)).astype(F32)
    return env.step(np.zeros((env.F * env.N, 2), F32))


def control_step(env: NumpyOracleEnv):
    """One control(i, env) of every formation: (vel [A, 2], obs, rew, done)."""
    v = control_velocity(env.p, env.g)
    obs, rew, done, _ = step_velocity(env, v)
    return v.reshape(-1, 2), obs, rew, done


# ----------------------------------------------------------------------------- fixtures
def case_names():
    return sorted(os.path.splitext(os.path.basename(p))[0]
                  for p in glob.glob(os.path.join(CONTROL_GOLDEN, "*.npz")))


def load_case(name: str) -> dict:
    z = np.load(os.path.join(CONTROL_GOLDEN, name + ".npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    F, N, goal, seed, steps = (int(v) for v in d["meta"])
    d.update(F=F, N=N, goal_in_obs=bool(goal), seed=seed, steps=steps, A=F * N, name=name)
    return d


def state_vec(px, py, gx, gy):
    ag = np.stack([px, py], axis=1).reshape(-1).astype(F32)
    gl = np.stack([gx, gy], axis=1).reshape(-1).astype(F32)
    return ag, gl


def check_step(case: dict, k: int, vel, obs, rew, done, px, py, gx, gy, t) -> None:
    """Hold step k (1-based) of a replay to the fixture: the six digests, and the full arrays
    where the fixture has them."""
    vel, obs, rew = (np.ascontiguousarray(v, F32) for v in (vel, obs, rew))
    done = np.ascontiguousarray(done).astype(np.bool_)
    ag, gl = state_vec(px, py, gx, gy)
    sel = {int(s): j for j, s in enumerate(case["sel_steps"])}
    if k in sel:
        j = sel[k]
        for name, got in (("vel", vel), ("obs", obs), ("rew", rew), ("agents", ag),
                          ("goal", gl)):
            np.testing.assert_array_equal(got.reshape(-1).view(np.uint32),
                                          case["sel_" + name][j].reshape(-1).view(np.uint32),
                                          err_msg=f"{case['name']}: {name} step {k}")
        np.testing.assert_array_equal(done, case["sel_done"][j], err_msg=f"done step {k}")
        np.testing.assert_array_equal(np.asarray(t, np.int32), case["sel_t"][j],
                                      err_msg=f"t step {k}")
    dig = case["digest"][k - 1]
    got = [d64(vel), d64(obs), d64(rew), d64(done), d64(ag), d64(gl, np.asarray(t, np.int32))]
    for name, a, b in zip(("vel", "obs", "reward", "done", "agents", "goal/t"), got, dig):
        assert a == b, f"{case['name']}: {name} digest step {k}"
