"""Timing of bioim_ik_solve (recorded, not gated).

n = 4096 frames made by tiling the 3D IK trial (tests/golden/ik_3D.npz), warm
start (OpenSim's q), tol 1e-9, cap 200; an evaluate-only call; VectorEnv.step
of the same model with N = 4096 in the same process; and the CPU yardstick
(tests/ik_reference.py, one thread) on a few frames.  Device events around each
call, median of 200 (10th-90th percentile), and the same 200 calls back to back
between one pair of events, per call.

    python tools/ik_timing.py [--n 4096] [--calls 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, 'bioimitation-gym_amd'), os.path.join(REPO, 'oracle'), os.path.join(REPO, 'tests')):
    sys.path.insert(0, p)


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
    ap.add_argument('--cpu-frames', type=int, default=8)
    args = ap.parse_args()
    import torch
    import oracle
    import ik_reference as R
    from bioimitation import _lib
    from bioimitation.inverse_kinematics import InverseKinematics
    from bioimitation.vector_env import VectorEnv
    oracle.build()
    z, mm = R.trial_model(oracle, '3D')
    env_id = str(z['env_id'])
    ik = InverseKinematics(env_id, mm.pairs())
    idx = np.arange(args.n) % len(z['q'])
    dev = lambda v: torch.as_tensor(v, device=ik.device, dtype=torch.float64).contiguous()  # noqa: E731
    x, w = dev(z['x_exp'][idx]), dev(z['weights'])
    q0 = dev(np.array([mm.qdof(z['q'][f]) for f in range(len(z['q']))])[idx])
    out = ik.solve(x, w, q0, tol=1e-9, max_iter=200, want=('q', 'status'))
    st = out['status'].cpu().numpy()
    wave = st.reshape(-1, 4).max(axis=1) if args.n % 4 == 0 else st
    res = dict(build_id=_lib.load().bioim_build_id().decode(), device=torch.cuda.get_device_name(0), n=args.n,
               env_id=env_id, markers=mm.nm, calls=args.calls,
               iterations=dict(min=int(st.min()), mean=float(st.mean()), max=int(st.max()),
                               wave_mean=float(wave.mean()), unfinished=int((st < 0).sum())))
    res['solve_warm'] = timed(lambda: ik.solve(x, w, q0, tol=1e-9, max_iter=200, want=('q', 'status')),
                              args.calls, torch)
    res['evaluate'] = timed(lambda: ik.evaluate(q0, x, w, want=('markers', 'err')), args.calls, torch)
    res['jacobian'] = timed(lambda: ik.evaluate(q0, want=('jacobian',)), args.calls, torch)
    env = VectorEnv(env_id, args.n, precision=64, seed=1000, auto_reset=True)
    env.reset()
    acts = torch.rand((args.n, env.action_dim), device=env.device, dtype=torch.float64)
    res['env_step'] = timed(lambda: env.step(acts), args.calls, torch)
    env.close()
    t0 = time.perf_counter()
    for f in range(0, args.cpu_frames * 6, 6):
        R.solve(mm, z['x_exp'][f], z['weights'], mm.qdof(z['q'][f]), tol=1e-9, max_iter=200)
    res['yardstick_cpu_ms_per_frame'] = (time.perf_counter() - t0) * 1e3 / args.cpu_frames
    ik.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
