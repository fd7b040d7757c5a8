"""The baseline formation controller, the reference's ``python simulate.py`` (README step 2).

Reference: simulate.py:256-319 ``control(i, env)`` -- a potential-field controller (springs to
the two ring neighbours and the opposite agent, attraction to a circle of radius 40 round the
goal) that steps one ``FormationSimulator`` with the velocity it computes -- and simulate.py
:321-329, which animates it on one formation of 10 agents for 1,000 frames.  It is the baseline
the RL policy is compared with.  Here the controller runs as HIP kernels over every formation of
a :class:`FormationEnv` (csrc/control_kernels.hip), bit for bit the reference's velocities.

    python marl-distributedformation_amd/baseline.py
    python marl-distributedformation_amd/baseline.py steps_to_simulate=200 save=baseline.gif
    python marl-distributedformation_amd/baseline.py evaluate=true num_formation=100000

Extra keys, as visualize_policy.py: ``steps_to_simulate`` (1000, simulate.py:322), ``save``
(write the animation to this file instead of opening a window), ``quiet`` (skip the per-step
prints); ``evaluate=true`` prints one JSON line of :func:`evaluate` over ``num_formation``
formations instead of drawing a figure.  ``num_agents_per_formation`` is 10 (simulate.py:324)
unless given on the command line; the controller needs it even (simulate.py:279).
"""
from __future__ import annotations

import json
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAUNCH_STEPS = 64  # steps per fused launch of evaluate()


def control(i, env):
    """simulate.py:256 ``control(i, env)`` with the batched env in place of one simulator: one
    controller step of EVERY formation of ``env`` (a :class:`FormationEnv`) through its numpy
    face.  ``i`` is the frame number FuncAnimation passes (unused, as in the reference).
    Returns what the reference's ``env.step`` call (:319) returns and ``control`` drops:
    ``(obs, rewards, dones, infos)``, aliasing the env's host buffers."""
    return env.step_velocity(env.control_tensor())


def evaluate(env, steps: int) -> dict:
    """Run ``steps`` controller steps of every formation as fused ``rollout_control`` launches
    and return the all-formation means of the eight ``env.metrics`` columns (final state; the
    ``reward`` column is the last step's) plus ``mean_reward``, the mean reward per agent-step
    over the whole run (from the launches' stats records, ``reduce_partials``)."""
    import torch

    steps = int(steps)
    if steps < 1:
        raise ValueError("steps must be >= 1")
    A, D, dev = env.num_envs, env.obs_dim, env.device
    L = min(steps, LAUNCH_STEPS)
    obs = torch.empty((L, A, D), dtype=torch.float32, device=dev)
    rew = torch.empty((L, A), dtype=torch.float32, device=dev)
    done = torch.empty((L, A), dtype=torch.bool, device=dev)
    partial = torch.zeros(2 * env.partial_count(), dtype=torch.float32, device=dev)
    total = torch.zeros(2, dtype=torch.float64, device=dev)
    part = torch.empty(2, dtype=torch.float64, device=dev)
    k, n = 0, L
    while k < steps:
        n = min(L, steps - k)
        env.rollout_control(n, obs=obs[:n], rew=rew[:n], done=done[:n], partial=partial)
        total += env.reduce_partials(partial, out=part)
        k += n
    sums = torch.empty(8, dtype=torch.float64, device=dev)
    env.metrics(rew=rew[n - 1], sums=sums)
    torch.cuda.current_stream(dev).synchronize()
    env.check()
    out = {name: float(v) / env.num_formation for name, v in zip(env.METRIC_NAMES, sums.tolist())}
    out["mean_reward"] = total.tolist()[0] / (float(A) * steps)
    return out


def _pkg():
    if _ROOT not in sys.path:
        sys.path.insert(0, _ROOT)
    import pkgload
    return pkgload.load()


def main(argv: list[str] | None = None):
    argv = list(sys.argv[1:] if argv is None else argv)
    from importlib import import_module
    pkg = _pkg()
    config = import_module(pkg.__name__ + ".config")
    venv = import_module(pkg.__name__ + ".vectorized_env")
    given = {a.split("=", 1)[0].lstrip("+").strip() for a in argv}
    if "num_agents_per_formation" not in given:
        argv.append("num_agents_per_formation=10")  # simulate.py:324
    cfg = config.load_config(overrides=argv)
    steps = int(cfg.get("steps_to_simulate", 1000))  # simulate.py:322
    if cfg.get("evaluate", False):
        env = venv.FormationEnv(cfg, visualize=False, log=False)
        res = evaluate(env, steps)
        res.update(steps=steps, num_formation=env.num_formation,
                   num_agents_per_formation=env.num_agents_per_formation)
        print(json.dumps(res))
        return res
    cfg.num_formation = 1  # simulate.py:324: one simulator
    env = venv.FormationEnv(cfg, visualize=True, log=False)
    verbose = not cfg.get("quiet", False)

    def frame(i):
        obs, rewards, dones, _ = control(i, env)
        if verbose:
            print("-" * 10)
            print(f"Step {i}")
            print(f"rewards: {rewards}")
            print(f"dones: {dones}")

    import matplotlib.animation as animation
    import matplotlib.pyplot as plt
    ani = animation.FuncAnimation(env.formationsim_list[0].fig, frame, frames=range(steps),
                                  interval=1)  # simulate.py:325-328
    out = cfg.get("save")
    if out:
        ani.save(str(out), writer="pillow" if str(out).endswith(".gif") else None)
    else:
        plt.show()
    return env


if __name__ == "__main__":
    main()
