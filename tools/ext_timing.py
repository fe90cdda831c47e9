"""Timing of the external-force step kernels (recorded, not
gated).

N = 4096 envs of Walking2D (config C3) and Running3D, fp64, auto-reset on: the
batched step with the default kernels, with a push table (the PERT kernels)
and with K = 2 external-force slots (torso and calcn_r, random wrenches), in
one process and one call.  Device events around each step, median of 200
(10th-90th percentile), and the same 200 steps back to back between one pair
of events, per step.

    python tools/ext_timing.py [--n 4096] [--calls 200]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'bioimitation-gym_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bk_timing import timed  # noqa: E402

MODELS = ('MuscleWalkingImitation2D-v0', 'MuscleRunningImitation3D-v0')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--calls', type=int, default=200)
    args = ap.parse_args()
    import torch
    from bioimitation import _lib
    from bioimitation.vector_env import VectorEnv
    res = dict(build_id=_lib.load().bioim_build_id().decode(), device=torch.cuda.get_device_name(0), n=args.n,
               calls=args.calls, models={})
    rng = np.random.default_rng(0)
    for env_id in MODELS:
        r = {}
        for kind in ('default', 'push', 'external_k2'):
            env = VectorEnv(env_id, args.n, precision=64, seed=1000, auto_reset=True)
            if kind == 'push':
                x = np.arange(0.0, 10.0, 0.03)
                env.set_perturbation(x, rng.choice([-50.0, 0.0, 50.0], size=(args.n, len(x))))
            elif kind == 'external_k2':
                w = rng.uniform(-50.0, 50.0, size=(args.n, 2, 9)) * np.array([1.0] * 3 + [0.002] * 3 + [0.2] * 3)
                env.set_external_forces(['torso', 'calcn_r'], torch.as_tensor(w, device=env.device, dtype=env.dtype))
            env.reset()
            acts = 0.4 * torch.rand((args.n, env.action_dim), device=env.device, dtype=env.dtype)
            r[kind] = timed(lambda: env.step(acts), args.calls, torch)
            env.close()
        res['models'][f'{env_id}/fp64'] = r
    print(json.dumps(res))


if __name__ == '__main__':
    main()
