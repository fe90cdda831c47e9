"""Timing of bioim_cmc (recorded, not gated).

n = 4096 own states of Walking2D and Running3D after five random steps (q, u,
activations and fiber lengths from the state rows), the target from q'' =
N(0, 2) through one bioim_id_eval launch: the library call with every output,
with the default output (excitation) alone, VectorEnv.computed_muscle_control
(gather + inverse dynamics + the call), CMCDrive's call, and VectorEnv.step of
the same model in the same process.  Device events around each call, median of
200 (10th-90th percentile), and the same 200 calls back to back between one
pair of events, per call.  The evaluation counts of the root solves are
reported with the figures.  fp64.

    python tools/cmc_timing.py [--n 4096] [--calls 200]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'bioimitation-gym_amd'))
sys.path.insert(0, os.path.join(REPO, 'tools'))

from bk_timing import MODELS, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--calls', type=int, default=200)
    args = ap.parse_args()
    import torch
    from bioimitation import _lib
    from bioimitation import computed_muscle_control as cmc
    from bioimitation.packdef import state_row_slices
    from bioimitation.vector_env import VectorEnv
    res = dict(build_id=_lib.load().bioim_build_id().decode(), device=torch.cuda.get_device_name(0), n=args.n,
               calls=args.calls, models={})
    for env_id in MODELS:
        env = VectorEnv(env_id, args.n, precision=64, seed=1000, auto_reset=True)
        pk = env.pack
        env.reset()
        acts = torch.rand((args.n, env.action_dim), device=env.device, dtype=env.dtype)
        for _ in range(5):
            env.step(acts)
        gen = torch.Generator(device=env.device).manual_seed(3)
        qdd = 2.0 * torch.randn((args.n, pk.ndof), device=env.device, dtype=torch.float64, generator=gen)
        first = env.computed_muscle_control(qdd=qdd, want=cmc.KEYS)
        rows = env.state_rows()
        sl, _ = state_row_slices(pk.ndof, pk.nmuscle, pk.nact, pk.horizon)
        q, u, act, lce = (rows[:, sl[f]].contiguous() for f in ('q', 'u', 'act', 'lce'))
        tau = first['tau']
        nsub = cmc.default_nsub(env, 0.01)
        call = lambda want: cmc.launch(env, q, u, act, lce, None, tau, None, 0.01, nsub, 0.0, 1.0, 1e-6, 30, want)  # noqa: E731
        again = call(cmc.KEYS)
        assert all(torch.equal(first[key], again[key]) for key in cmc.KEYS)
        rs, st = first['root_status'], first['status']
        r = dict(nsub=nsub, solver_passes_max=int(st.max()), solver_passes_mean=float(st.double().mean()),
                 solver_failed=int((st < 0).sum()), root_cap_hit=int((rs < 0).sum()),
                 root_on_bound_share=float((rs == 0).double().mean()), root_evals_max=int(rs.max()),
                 root_evals_mean_solved=float(rs[rs > 0].double().mean()))
        drive = cmc.CMCDrive(env)
        r['call_all'] = timed(lambda: call(cmc.KEYS), args.calls, torch)
        r['call_default'] = timed(lambda: call(cmc.DEFAULT_WANT), args.calls, torch)
        r['env_computed_muscle_control'] = timed(lambda: env.computed_muscle_control(qdd=qdd), args.calls, torch)
        r['cmc_drive'] = timed(drive, args.calls, torch)
        r['env_step'] = timed(lambda: env.step(acts), args.calls, torch)
        res['models'][f'{env_id}/fp64'] = r
        env.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
