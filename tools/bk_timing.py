"""Timing of bioim_body_kin (recorded, not gated).

n = 4096 states of Walking2D and Running3D, taken from the envs themselves
after a few random steps (q, u from the state rows, q'' from a REALIZE
report): the library call with every output and the contact spheres as points,
with the default outputs (com, system) alone, VectorEnv.body_kinematics
(gather + the call), and VectorEnv.step of the same model in the same process.
Device events around each call, median of 200 (10th-90th percentile), and the
same 200 calls back to back between one pair of events, per call.  fp64.

    python tools/bk_timing.py [--n 4096] [--calls 200]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'bioimitation-gym_amd'))

MODELS = ('MuscleWalkingImitation2D-v0', 'MuscleRunningImitation3D-v0')


def timed(fn, calls, torch):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    ms = np.array(ms)
    return dict(median_ms=float(np.median(ms)), p10_ms=float(np.percentile(ms, 10)),
                p90_ms=float(np.percentile(ms, 90)), back_to_back_ms=a.elapsed_time(b) / calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--calls', type=int, default=200)
    args = ap.parse_args()
    import torch
    from bioimitation import _lib
    from bioimitation import body_kinematics as bk
    from bioimitation.obslayout import load_names
    from bioimitation.packdef import state_row_slices
    from bioimitation.refmotion import sphere_points
    from bioimitation.vector_env import VectorEnv
    res = dict(build_id=_lib.load().bioim_build_id().decode(), device=torch.cuda.get_device_name(0), n=args.n,
               calls=args.calls, models={})
    for env_id in MODELS:
        env = VectorEnv(env_id, args.n, precision=64, seed=1000, auto_reset=True)
        pk = env.pack
        bodies = list(load_names(env_id)['bodies'])
        env.reset()
        acts = torch.rand((args.n, env.action_dim), device=env.device, dtype=env.dtype)
        for _ in range(5):
            env.step(acts)
        pts, _ = sphere_points(pk, bodies)
        first = env.body_kinematics(qdd='own', points=pts, want=bk.KEYS)       # also fills the REALIZE report
        rows = env.state_rows()
        sl, _ = state_row_slices(pk.ndof, pk.nmuscle, pk.nact, pk.horizon)
        q, u = (rows[:, sl[f]].to(env.dtype).contiguous() for f in ('q', 'u'))
        dof_coord = [c for d in range(pk.ndof) for c in range(pk.ncoord) if pk.coord[c].dof == d]
        k = 2 + 2 * pk.ncoord
        qdd = env.osim_report[:, k:k + pk.ncoord][:, dof_coord].contiguous()
        pt_body, pt_local = bk.check_points(bodies, pts)
        call = lambda want: bk.launch(env, q, u, qdd, pt_body, pt_local, False, want)  # noqa: E731
        again = call(bk.KEYS)
        assert all(torch.equal(first[key], again[key]) for key in bk.KEYS)
        r = dict(points=len(pts))
        r['call_all'] = timed(lambda: call(bk.KEYS), args.calls, torch)
        r['call_default'] = timed(lambda: call(bk.DEFAULT_WANT), args.calls, torch)
        r['env_body_kinematics'] = timed(lambda: env.body_kinematics(), args.calls, torch)
        r['env_step'] = timed(lambda: env.step(acts), args.calls, torch)
        res['models'][f'{env_id}/fp64'] = r
        env.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
