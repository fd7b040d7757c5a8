"""Generate the baseline-controller fixtures by running the REFERENCE's control() (build
container only).

Run from the repo root in the build container (where /root/reference exists):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/gen_golden_control.py

The reference is imported with the stub recipe of gen_golden.py.  Per case: torch.manual_seed(seed),
the reference FormationEnv (its ctor consumes draw set 1), env.reset() (draw set 2), then every
step simulate.control(k, sim) for each sim of env.formationsim_list, in order.  A recording
wrapper set as each instance's ``step`` captures the velocity control() hands to it and what the
simulator's step returns.

Output: tests/golden/control/<case>.npz -- DATA only.  (A sub-directory: golden_util.case_names()
globs tests/golden/*.npz, whose schema is another.)

Per case:
  meta            int64 [F, N, goal_in_obs, seed, steps]
  dd              float32 the controller's desired neighbour distance, pi * 40 / N
                  (simulate.py:286), as it meets the fp32 tensors
  state_reset     float32 [A*2 + F*2] agents + goals after env.reset()
  digest          uint64 [steps, 6] blake2b-64 of (vel, obs, reward, done, agents, goal|t bytes)
  sel_steps       int64 [k] 1-based step numbers with full arrays below
  sel_vel/sel_obs/sel_rew/sel_done/sel_agents/sel_goal/sel_t
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402  (the stub recipe, _d64, REF)

OUT = os.path.join(HERE, "control")

CASES = [
    # name,          F,  N,    goal,  seed, steps
    ("f3_n2_d8",     3,  2,    True,  101,  1010),   # smallest N
    ("f7_n4_d6",     7,  4,    False, 102,  40),
    ("f13_n10_d8",   13, 10,   True,  103,  1010),   # 6 per wave, last wave partial, reset
    ("f11_n12_d8",   11, 12,   True,  104,  30),     # 4 idle lanes per wave
    ("f2_n64_d8",    2,  64,   True,  105,  1010),   # full wave
    ("f2_n66_d6",    2,  66,   False, 106,  30),     # smallest block-path size
    ("f2_n100_d8",   2,  100,  True,  107,  1010),   # block path across the reset
    ("f1_n1024_d8",  1,  1024, True,  108,  12),
]

SEL = [1, 2, 3, 500, 1001, 1002, 1003]


def run_case(name, F, N, goal, seed, steps):
    import torch
    from types import SimpleNamespace
    import simulate
    import vectorized_env

    torch.manual_seed(seed)
    cfg = SimpleNamespace(num_formation=F, num_agents_per_formation=N, goal_in_obs=goal,
                          share_reward_ratio=0.25, name="golden")
    env = vectorized_env.FormationEnv(cfg, visualize=False, log=False)
    sims = env.formationsim_list
    env.reset()

    def state():
        ag = np.concatenate([s.agents.numpy().reshape(-1) for s in sims])
        gl = np.concatenate([s.goal.numpy().reshape(-1) for s in sims])
        t = np.array([s.steps_since_reset for s in sims], np.int32)
        return ag.astype(np.float32), gl.astype(np.float32), t

    ag, gl, _ = state()
    state_reset = np.concatenate([ag, gl])

    rec = {}

    def wrap(idx, sim):
        inner = sim.step  # the class's bound method

        def step(v):
            vel = v.detach().clone().numpy()
            obs, rew, done, _ = inner(v)
            rec[idx] = (vel, obs.numpy().copy(), rew.numpy().copy(), bool(done))
            return obs, rew, done, {}
        sim.step = step

    for idx, sim in enumerate(sims):
        wrap(idx, sim)

    digest = np.zeros((steps, 6), np.uint64)
    sel = [s for s in SEL if s <= steps]
    out_sel = {k: [] for k in ("vel", "obs", "rew", "done", "agents", "goal", "t")}
    dones = 0
    for k in range(1, steps + 1):
        rec.clear()
        for sim in sims:
            simulate.control(k, sim)
        vel = np.concatenate([rec[i][0] for i in range(F)]).astype(np.float32)
        obs = np.concatenate([rec[i][1] for i in range(F)]).astype(np.float32)
        rew = np.concatenate([rec[i][2] for i in range(F)]).astype(np.float32)
        done = np.repeat(np.array([rec[i][3] for i in range(F)], np.bool_), N)
        assert vel.shape == (F * N, 2) and obs.shape == (F * N, 8 if goal else 6)
        assert not np.isnan(vel).any()
        ag, gl, t = state()
        digest[k - 1] = [gg._d64(vel), gg._d64(obs), gg._d64(rew), gg._d64(done), gg._d64(ag),
                         gg._d64(gl, t)]
        dones += int(done.any())
        if k in sel:
            for key, v in zip(out_sel, (vel, obs, rew, done, ag, gl, t)):
                out_sel[key].append(v)
    out = dict(
        meta=np.array([F, N, int(goal), seed, steps], np.int64),
        dd=np.float32(np.pi * 40 / N),
        state_reset=state_reset, digest=digest, sel_steps=np.array(sel, np.int64),
        sel_vel=np.array(out_sel["vel"], np.float32), sel_obs=np.array(out_sel["obs"], np.float32),
        sel_rew=np.array(out_sel["rew"], np.float32),
        sel_done=np.array(out_sel["done"], np.bool_),
        sel_agents=np.array(out_sel["agents"], np.float32),
        sel_goal=np.array(out_sel["goal"], np.float32), sel_t=np.array(out_sel["t"], np.int32),
    )
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: F={F} N={N} steps={steps} done steps={dones} "
          f"{os.path.getsize(path)} bytes", flush=True)


def main(argv):
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.dont_write_bytecode = True
    gg._install_stubs()
    sys.path.insert(0, gg.REF)
    want = set(argv[1:])
    for c in CASES:
        if want and c[0] not in want:
            continue
        run_case(*c)


if __name__ == "__main__":
    main(sys.argv)
