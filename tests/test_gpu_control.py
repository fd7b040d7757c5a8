"""GPU: the baseline formation controller (csrc/control_kernels.hip) against the fixtures the
reference's own control() produced (tests/golden/control), and the velocity step against the
existing env fixtures.  fp32 results must match bit for bit; dones exactly."""
import os

import numpy as np
import pytest
import torch

import control_oracle as co
import golden_util as gu
from oracle import synth_actions

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = co.case_names()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def make_env(venv, F, N, goal=True, seed=0, **kw):
    cfg = {"num_formation": F, "num_agents_per_formation": N, "goal_in_obs": goal}
    return venv.FormationEnv(cfg, device=DEV, seed=seed, **kw)


def host_state(env):
    return tuple(v.cpu().numpy() for v in env.get_state())


# ------------------------------------------------------------------ 1. fixture replay
@pytest.mark.parametrize("chunk", [1, 64])
@pytest.mark.parametrize("name", CASES)
def test_control_fixture_replay(venv, name, chunk):
    """Every control fixture on HIP in MT19937 mode through rollout_control launches of `chunk`
    steps.  chunk = 1 holds all six digests (and the selected arrays) at every step; chunk = 64
    holds vel / obs / reward / done at every step and the state at every launch end (the state of
    a fused launch's inner steps stays on chip)."""
    c = co.load_case(name)
    assert len(CASES) == 8
    env = make_env(venv, c["F"], c["N"], c["goal_in_obs"], c["seed"])
    env.reset()
    px, py, gx, gy, t = host_state(env)
    ag, gl = co.state_vec(px, py, gx, gy)
    assert np.array_equal(bits(np.concatenate([ag, gl])), bits(c["state_reset"])), "reset state"
    A = c["A"]
    sel = {int(s): j for j, s in enumerate(c["sel_steps"])}
    k = 0
    while k < c["steps"]:
        T = min(chunk, c["steps"] - k)
        vel = torch.empty((T, A, 2), dtype=torch.float32, device=DEV)
        obs, rew, done = env.rollout_control(T, vel_out=vel)
        vel, obs, rew, done = (v.cpu().numpy() for v in (vel, obs, rew, done))
        st = host_state(env)
        for j in range(T):
            kk = k + j + 1
            if j == T - 1:
                co.check_step(c, kk, vel[j], obs[j], rew[j], done[j], *st)
                continue
            dig = c["digest"][kk - 1]
            assert gu.d64(vel[j]) == dig[0], f"vel digest step {kk}"
            assert gu.d64(obs[j]) == dig[1], f"obs digest step {kk}"
            assert gu.d64(rew[j]) == dig[2], f"reward digest step {kk}"
            assert gu.d64(done[j].astype(np.bool_)) == dig[3], f"done digest step {kk}"
            if kk in sel:
                s = sel[kk]
                for nm, got in (("vel", vel[j]), ("obs", obs[j]), ("rew", rew[j])):
                    np.testing.assert_array_equal(bits(got).reshape(-1),
                                                  bits(c["sel_" + nm][s]).reshape(-1),
                                                  err_msg=f"{nm} step {kk}")
                np.testing.assert_array_equal(done[j], c["sel_done"][s])
        k += T
    env.check()


# ------------------------------------------------------------------ 2. velocity face, old fixtures
@pytest.mark.parametrize("name,chunk", [("f1_n5_d8_walls", 64), ("f4_n3_d6_extreme", 7),
                                        ("f13_n5_d8_short", 7)])
def test_env_fixtures_through_velocity_face(venv, name, chunk):
    """The reference env's own fixtures (walls, extreme action values, odd N) replayed through
    rollout_velocity with v = float32(10) * action computed on the host: vectorized_env.py:70
    does that product in fp32 before FormationSimulator.step sees it, so the bits must match."""
    c = gu.load_case(name)
    env = make_env(venv, c["F"], c["N"], c["goal_in_obs"], c["seed"])
    assert np.array_equal(bits(env.reset()), bits(c["obs_reset"]))
    A = c["A"]
    sel = {int(s): j for j, s in enumerate(c["sel_steps"])}
    k = 0
    while k < c["steps"]:
        T = min(chunk, c["steps"] - k)
        with np.errstate(over="ignore"):
            v = np.stack([np.float32(10) * synth_actions(c["act_seed"], k + j + 1, A, c["amp"])
                          for j in range(T)]).astype(np.float32)
        obs, rew, done = env.rollout_velocity(torch.from_numpy(v).to(DEV))
        obs, rew, done = (x.cpu().numpy() for x in (obs, rew, done))
        for j in range(T):
            kk = k + j + 1
            dig = c["digest"][kk - 1]
            if kk in sel:
                s = sel[kk]
                np.testing.assert_array_equal(bits(obs[j]), bits(c["sel_obs"][s]),
                                              err_msg=f"obs step {kk}")
                np.testing.assert_array_equal(bits(rew[j]), bits(c["sel_rew"][s]),
                                              err_msg=f"reward step {kk}")
                np.testing.assert_array_equal(done[j], c["sel_done"][s])
            assert gu.d64(obs[j]) == dig[0], f"obs digest step {kk}"
            assert gu.d64(rew[j]) == dig[1], f"reward digest step {kk}"
            assert gu.d64(done[j].astype(np.bool_)) == dig[2], f"done digest step {kk}"
        k += T
        px, py, gx, gy, t = host_state(env)
        ag, gl = co.state_vec(px, py, gx, gy)
        dig = c["digest"][k - 1]
        assert gu.d64(ag) == dig[3], f"agents digest step {k}"
        assert gu.d64(gl, t.astype(np.int32)) == dig[4], f"goal/t digest step {k}"
    env.check()


# ------------------------------------------------------------------ 3. fused == unfused
@pytest.mark.parametrize("F,N", [(13, 10), (27, 6), (3, 66)])
def test_fused_equals_unfused(venv, F, N):
    """rollout_control(7) == 7 x (control_tensor + step_velocity_tensor), bit for bit, in Philox
    mode with max_steps = 4, so the launch holds an auto-reset; its stats records equal those of
    rollout_velocity fed the same velocities from the same state."""
    T, A = 7, F * N
    kw = dict(seed=5, reset_mode="philox", max_steps=4)
    fused, loop, fed = (make_env(venv, F, N, **kw) for _ in range(3))
    n = fused.partial_count()
    pa = torch.full((2 * n,), -7.0, dtype=torch.float32, device=DEV)
    pc = torch.full((2 * n,), -9.0, dtype=torch.float32, device=DEV)
    vel = torch.empty((T, A, 2), dtype=torch.float32, device=DEV)
    obs, rew, done = fused.rollout_control(T, vel_out=vel, partial=pa)
    assert bool(done.any()) and not bool(done.all()), "the launch must hold a reset"
    for k in range(T):
        v = loop.control_tensor()
        o, r, d = loop.step_velocity_tensor(v)
        assert torch.equal(v.view(torch.int32), vel[k].view(torch.int32)), f"vel step {k}"
        assert torch.equal(o.view(torch.int32), obs[k].view(torch.int32)), f"obs step {k}"
        assert torch.equal(r.view(torch.int32), rew[k].view(torch.int32)), f"rew step {k}"
        assert torch.equal(d, done[k]), f"done step {k}"
    for a, b in zip(fused.get_state(), loop.get_state()):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "final state"
    o2, r2, d2 = fed.rollout_velocity(vel, partial=pc)
    assert torch.equal(o2.view(torch.int32), obs.view(torch.int32))
    assert torch.equal(r2.view(torch.int32), rew.view(torch.int32))
    assert torch.equal(d2, done)
    assert torch.equal(pa.view(torch.int32), pc.view(torch.int32)), "stats records"
    tot = fused.reduce_partials(pa).cpu().numpy()
    assert tot[1] == float(done.sum().item())
    # without vel_out the same results
    again = make_env(venv, F, N, **kw)
    o3, r3, d3 = again.rollout_control(T)
    assert torch.equal(o3.view(torch.int32), obs.view(torch.int32))
    assert torch.equal(r3.view(torch.int32), rew.view(torch.int32))


# ------------------------------------------------------------------ 4. control_tensor reads only
@pytest.mark.parametrize("F,N", [(13, 10), (3, 66)])
def test_control_tensor_leaves_state_unchanged(venv, F, N):
    env = make_env(venv, F, N, seed=3)
    env.reset()
    before = [v.clone() for v in env.get_state()]
    out = torch.empty((F * N, 2), dtype=torch.float32, device=DEV)
    v = env.control_tensor(out)
    assert v is out and bool(torch.isfinite(v).all())
    for a, b in zip(before, env.get_state()):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    px, py, gx, gy, _ = host_state(env)
    want = co.control_velocity(np.stack([px, py], 1).reshape(F, N, 2), np.stack([gx, gy], 1))
    np.testing.assert_array_equal(bits(v.cpu().numpy()), bits(want.reshape(-1, 2)))


# ------------------------------------------------------------------ 5. sharding
def test_shards_reproduce_unsharded_rows(venv):
    F, N, T = 13, 10, 7
    kw = dict(seed=11, reset_mode="philox", max_steps=4)
    whole = make_env(venv, F, N, **kw)
    vel = torch.empty((T, F * N, 2), dtype=torch.float32, device=DEV)
    obs, rew, done = whole.rollout_control(T, vel_out=vel)
    for f0, cnt in ((0, 5), (5, 8)):
        sh = make_env(venv, cnt, N, first_formation=f0, total_formations=F, **kw)
        sv = torch.empty((T, cnt * N, 2), dtype=torch.float32, device=DEV)
        so, sr, sd = sh.rollout_control(T, vel_out=sv)
        rows = slice(f0 * N, (f0 + cnt) * N)
        assert torch.equal(sv.view(torch.int32), vel[:, rows].view(torch.int32))
        assert torch.equal(so.view(torch.int32), obs[:, rows].view(torch.int32))
        assert torch.equal(sr.view(torch.int32), rew[:, rows].view(torch.int32))
        assert torch.equal(sd, done[:, rows])
        one = sh.control_tensor()
        ref = whole.control_tensor()[rows]
        assert torch.equal(one.view(torch.int32), ref.view(torch.int32))


# ------------------------------------------------------------------ 6. rejected sizes
def test_odd_and_large_formations_rejected(venv, flib):
    odd = make_env(venv, 3, 5, seed=1, reset_mode="philox")
    with pytest.raises(flib.FenvError, match="even num_agents"):
        odd.control_tensor()
    with pytest.raises(flib.FenvError, match="even num_agents"):
        odd.rollout_control(2)
    obs, rew, done = odd.rollout_velocity(torch.zeros((2, 15, 2), device=DEV))  # odd N is fine
    assert obs.shape == (2, 15, 8)
    big = make_env(venv, 1, 1026, seed=1, reset_mode="philox")
    with pytest.raises(flib.FenvError, match="above 1024 agents"):
        big.control_tensor()
    with pytest.raises(flib.FenvError, match="above 1024 agents"):
        big.rollout_control(1)
    with pytest.raises(flib.FenvError, match="above 1024 agents"):
        big.rollout_velocity(torch.zeros((1, 1026, 2), device=DEV))
    with pytest.raises(AssertionError):
        odd.rollout_velocity(torch.zeros((2, 14, 2), device=DEV))


# ------------------------------------------------------------------ 7. python module
@pytest.fixture(scope="module")
def baseline(pkg):
    from importlib import import_module
    return import_module(pkg.__name__ + ".baseline")


def test_baseline_control_matches_fixture(venv, baseline):
    c = co.load_case("f13_n10_d8")
    env = make_env(venv, c["F"], c["N"], c["goal_in_obs"], c["seed"])
    env.reset()
    for k in (1, 2, 3):
        obs, rew, done, infos = baseline.control(k, env)
        assert len(infos) == c["A"]
        j = int(np.nonzero(c["sel_steps"] == k)[0][0])
        np.testing.assert_array_equal(bits(obs), bits(c["sel_obs"][j]))
        np.testing.assert_array_equal(bits(rew), bits(c["sel_rew"][j]))
        np.testing.assert_array_equal(done, c["sel_done"][j])
        px, py, gx, gy, t = host_state(env)
        ag, gl = co.state_vec(px, py, gx, gy)
        np.testing.assert_array_equal(bits(ag), bits(c["sel_agents"][j]))


def test_step_velocity_takes_numpy(venv):
    """The numpy face with a host array (copied into the env's device-mapped block), and its
    shape check (simulate.py:79)."""
    c = co.load_case("f11_n12_d8")
    env = make_env(venv, c["F"], c["N"], c["goal_in_obs"], c["seed"])
    env.reset()
    for k in (1, 2, 3):
        v = env.control_tensor().cpu().numpy()
        obs, rew, done, _ = env.step_velocity(v)
        co.check_step(c, k, v, obs, rew, done, *host_state(env))
    with pytest.raises(AssertionError):
        env.step_velocity(np.zeros((c["A"] - 1, 2), np.float32))


def test_baseline_evaluate(venv, baseline):
    """70 steps = two launches (64 + 6).  mean_reward comes from fp32 stats records: each is a
    chain of at most 64 per-lane adds, 6 wave-reduction adds and 3 workgroup adds, later summed
    in double, so it differs from the float64 mean of the reward buffer by at most
    73 * 2^-24 * mean|r|."""
    F, N, steps = 13, 10, 70
    kw = dict(seed=21, reset_mode="philox")
    res = baseline.evaluate(make_env(venv, F, N, **kw), steps)
    names = venv.FormationEnv.METRIC_NAMES
    assert set(names) | {"mean_reward"} <= set(res)
    assert all(np.isfinite(res[k]) for k in names + ("mean_reward",))
    _, rew, _ = make_env(venv, F, N, **kw).rollout_control(steps)
    r = rew.double()
    bound = 73 * 2.0 ** -24 * float(r.abs().mean())
    assert abs(res["mean_reward"] - float(r.mean())) <= bound


def test_baseline_main_saves_animation(baseline, tmp_path):
    import matplotlib
    matplotlib.use("Agg")
    out = tmp_path / "baseline.gif"
    baseline.main(["steps_to_simulate=3", f"save={out}", "quiet=true"])
    assert os.path.getsize(out) > 0
