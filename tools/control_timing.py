"""Timing of the fused baseline-controller rollout on one device, one process.

Philox mode, T = 10, at 65,536 x 10 and 16,384 x 64 (BASELINE configs 2 and 4).  Three things are
alternated, `reps` (default 200) timed launches each after warm-up, every launch bracketed by
its own pair of device events:

  control   rollout_control(T) without vel_out      (k_control_rollout_wave)
  random    rollout_random(T) on the same env       (the existing kernel: the yardstick)
  unfused   T x (control_tensor + step_velocity_tensor)

One JSON line per config: median and min ms per launch, agent-steps/s, the algorithmic bytes
(DESIGN §4.1's B_roll without the action bytes: 4 D + 5 per agent-step, 16 + 20 / N per agent per
launch) over the median time as a share of the 8 TB/s HBM spec, and the two ratios
control / random and unfused / control.

    python tools/control_timing.py [reps]
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pkgload  # noqa: E402

pkg = pkgload.load()
from importlib import import_module  # noqa: E402

venv = import_module(pkg.__name__ + ".vectorized_env")
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
T, D = 10, 8
HBM_SPEC = 8.0e12
dev = torch.device("cuda", 0)


def run(F, N):
    A = F * N
    cfg = {"num_formation": F, "num_agents_per_formation": N, "goal_in_obs": True}
    env = venv.FormationEnv(cfg, log=False, device=dev, seed=1, reset_mode="philox")
    obs = torch.empty((T, A, D), dtype=torch.float32, device=dev)
    rew = torch.empty((T, A), dtype=torch.float32, device=dev)
    done = torch.empty((T, A), dtype=torch.bool, device=dev)
    vel = torch.empty((A, 2), dtype=torch.float32, device=dev)
    step = [0]

    def control():
        env.rollout_control(T, obs=obs, rew=rew, done=done)

    def random():
        env.rollout_random(T, act_seed=3, step_offset=step[0], obs=obs, rew=rew, done=done)
        step[0] += T

    def unfused():
        for k in range(T):
            env.control_tensor(vel)
            env.step_velocity_tensor(vel, obs=obs[k], rew=rew[k], done=done[k])

    fns = {"control": control, "random": random, "unfused": unfused}
    for _ in range(5):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    for _ in range(REPS):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            ev[name].append((a, b))
    torch.cuda.synchronize()
    env.check()
    out = {"F": F, "N": N, "T": T, "reps": REPS, "kernel_random": env.rollout_kernel_name(T)}
    bytes_launch = A * (T * (4 * D + 5) + 16 + 20.0 / N)
    out["algorithmic_bytes_per_launch"] = bytes_launch
    for name, pairs in ev.items():
        ms = [a.elapsed_time(b) for a, b in pairs]
        med = statistics.median(ms)
        out[name] = {"ms_median": med, "ms_min": min(ms),
                     "agent_steps_per_s": A * T / (med * 1e-3)}
        if name != "unfused":
            out[name]["hbm_share"] = bytes_launch / (med * 1e-3) / HBM_SPEC
    out["control_over_random"] = out["control"]["ms_median"] / out["random"]["ms_median"]
    out["unfused_over_control"] = out["unfused"]["ms_median"] / out["control"]["ms_median"]
    print(json.dumps(out), flush=True)
    env.release()


for F, N in ((65536, 10), (16384, 64)):
    run(F, N)
