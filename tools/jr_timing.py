"""Timing of bioim_joint_reaction (recorded, not gated).

n = 4096 states of Walking2D and Running3D, taken from the envs themselves
after a few random steps (q, u from the state rows, q'' and tendon forces from
a REALIZE report): the library call with every output, with `reaction` alone,
VectorEnv.joint_reaction (gather + REALIZE + the call), and VectorEnv.step of
the same model in the same process.  Device events around each call, median of
200 (10th-90th percentile), and the same 200 calls back to back between one
pair of events, per call.  fp64 and fp32.

    python tools/jr_timing.py [--n 4096] [--calls 200]
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
    from bioimitation import joint_reaction as jr
    from bioimitation.packdef import state_row_slices
    from bioimitation.vector_env import VectorEnv
    res = dict(build_id=_lib.load().bioim_build_id().decode(), device=torch.cuda.get_device_name(0), n=args.n,
               calls=args.calls, models={})
    for env_id in MODELS:
        for precision in (64, 32):
            env = VectorEnv(env_id, args.n, precision=precision, seed=1000, auto_reset=True)
            pk = env.pack
            env.reset()
            acts = torch.rand((args.n, env.action_dim), device=env.device, dtype=env.dtype)
            for _ in range(5):
                env.step(acts)
            first = env.joint_reaction(want=jr.KEYS)            # also fills the REALIZE report
            rows = env.state_rows()
            sl, _ = state_row_slices(pk.ndof, pk.nmuscle, pk.nact, pk.horizon)
            q, u = (rows[:, sl[f]].to(env.dtype).contiguous() for f in ('q', 'u'))
            coord_of = [c for d in range(pk.ndof) for c in range(pk.ncoord) if pk.coord[c].dof == d]
            k = 2 + 2 * pk.ncoord
            qdd = env.osim_report[:, k:k + pk.ncoord][:, coord_of].contiguous()
            k = 2 + 3 * pk.ncoord + 18 * pk.nosbody + 9
            ft = env.osim_report[:, k:k + 7 * pk.nmuscle].reshape(args.n, pk.nmuscle, 7)[:, :, 6].contiguous()
            again = jr.launch(env, q, u, qdd, ft, None, True, 'child', 'child', jr.KEYS)
            assert all(torch.equal(first[key], again[key]) for key in jr.KEYS)
            r = dict(hip_r_load_N=float(first['reaction'][:, 1, :3].norm(dim=1).median()))
            r['call_all_outputs'] = timed(lambda: jr.launch(env, q, u, qdd, ft, None, True, 'child', 'child', jr.KEYS),
                                          args.calls, torch)
            r['call_reaction'] = timed(lambda: jr.launch(env, q, u, qdd, ft, None, True, 'child', 'child', ('reaction',)),
                                       args.calls, torch)
            r['env_joint_reaction'] = timed(lambda: env.joint_reaction(), args.calls, torch)
            r['env_step'] = timed(lambda: env.step(acts), args.calls, torch)
            res['models'][f'{env_id}/fp{precision}'] = r
            env.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
