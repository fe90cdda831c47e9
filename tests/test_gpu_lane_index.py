"""The per-lane index record of the planar step kernels' dynamics call
(csrc/bioim_kinematics.h, LaneIdx / BIOIM_LANEIDX: the dof lane's parent-frame
offset and body, its TAU gather list and limit mask, the limit lane's
coordinate and the muscle lane's path-point numbers, read once per launch into
packed registers instead of once per call).

What can go wrong with it: a lane past a count (no dof, limit or muscle of its
own) unpacking a value the old code never formed; a field too narrow for a
model's value; a record built for one model used for another; a record that
is wrong at a later call of its launch (after the report's LDS staging, the
reset realize) or at a later step of a fused rollout, which runs the step's
prologue, the record's build included, once per step.

Bounds: observation, reward and info against the fp64 oracle at the suite's
5e-9 of max(|x|, 1) (reward absolute), for reset, one-step and the 12-step
free-running states alike, done equal; the same arithmetic run twice, bitwise."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason='needs a HIP GPU')]

M2D, T2D = 'MuscleWalkingImitation2D-v0', 'TorqueWalkingImitation2D-v0'
MLK2D, TLK2D = 'MuscleLockedKneeImitation2D-v0', 'TorqueLockedKneeImitation2D-v0'
MR2D = 'MuscleRunningImitation2D-v0'
PLANAR = [M2D, T2D, MLK2D, TLK2D]
SEED = 21
TOL = 5e-9


def _rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def _env(env_id, n, auto_reset=False, **kw):
    from bioimitation.vector_env import VectorEnv
    return VectorEnv(env_id, n, precision=64, seed=SEED, auto_reset=auto_reset, **kw)


def _oracle(env_id, n):
    import oracle
    from bioimitation.registry import load_pack
    pk = load_pack(env_id)
    orc = oracle.Oracle(pk)
    return pk, orc, orc.new_envs(n)


def _actions(pk, rng, rows):
    """muscle excitations U[0, 1]; torque models: PD targets of the next
    reference row + N(0, 0.05)"""
    n = len(rows)
    if pk.nmuscle:
        return rng.uniform(0.0, 1.0, size=(n, pk.nact))
    base = np.array([[pk.ref_q[min(int(r) + 1, pk.nrows - 1)][pk.pd_coord[a]] for a in range(pk.nact)] for r in rows])
    return base + rng.normal(0.0, 0.05, size=(n, pk.nact))


def _cat(out):
    import torch
    o, r, d, inf = out
    return torch.cat([o, r[:, None], d[:, None].to(o.dtype), inf], 1).clone()


@pytest.mark.parametrize('env_id', PLANAR)
def test_lanes_past_counts_and_partial_workgroup(env_id):
    """40 envs (two full workgroups of 16 and a half-filled one), 12
    auto-reset steps from rows that end episodes inside the run: every env and
    step against the oracle (done equal; the step's own observation through
    final_obs, reward, info), a reset's observation against the oracle reset
    at the row the launch drew.  Covers lanes 14-15 of the muscle pass, lanes
    >= ND in phase 3, lanes >= NL in the limits, the reset realize and the
    cached first substep's gather."""
    import torch
    n, steps = 40, 12
    pk, orc, bufs = _oracle(env_id, n)
    env = _env(env_id, n, auto_reset=True)
    env.enable_final_obs()
    start = [pk.n_episode - 3, pk.nrows - 2, pk.reset_hi // 2, pk.n_episode - 6, 7]
    rows = np.array([start[i % len(start)] for i in range(n)], dtype=np.int32)
    rng = np.random.default_rng(8)
    obs0 = env.reset(ref_index=rows).cpu().numpy()
    for i in range(n):
        e = _rel(obs0[i], orc.reset(bufs, i, int(rows[i]))).max()
        assert e < TOL, (i, e)
    ref_istep = np.array(pk.ref_istep[:pk.nrows])
    worst, worst_reset, resets = 0.0, 0.0, 0
    for t in range(steps):
        acts = _actions(pk, rng, rows + t)
        obs, rew, done, info = env.step(torch.as_tensor(acts, device=env.device))
        torch.cuda.synchronize()
        obs, rew, done, info, fin = (x.cpu().numpy() for x in (obs, rew, done, info, env.final_obs))
        state = env.get_state()
        for i in range(n):
            o, r, d, inf = orc.step(bufs, i, acts[i])
            e = max(_rel(fin[i], o).max(), abs(rew[i] - r), _rel(info[i], inf).max())
            assert bool(done[i]) == d, (t, i)
            assert e < TOL, (t, i, e)
            worst = max(worst, e)
            if not d:
                assert np.array_equal(obs[i], fin[i]), (t, i)
                continue
            resets += 1
            cand = [int(c) for c in np.where(ref_istep[:pk.reset_hi + 1] == int(state[i, 1]))[0]]
            errs = [_rel(obs[i], orc.reset(bufs, i, c)).max() for c in cand]
            assert cand and min(errs) < TOL, (t, i, state[i, 1], cand, errs)
            worst_reset = max(worst_reset, min(errs))
            orc.reset(bufs, i, cand[int(np.argmin(errs))])
    print(f'{env_id}: {steps} steps x {n} envs, max rel err {worst:.2e}; {resets} resets in a launch, '
          f'max rel err of their observation {worst_reset:.2e}')
    assert resets >= 1
    env.close()


def _point_cases(pk):
    """(dof, coordinate value) pairs that put every conditional path point's
    coordinate below, inside and above its range, and every moving point's
    function argument below, inside and above its knots"""
    cases = []

    def add(coord, lo, hi):
        dof = pk.coord[coord].dof
        if dof < 0:
            return
        for v in (lo - 0.15, 0.5 * (lo + hi), hi + 0.15):
            if not any(d == dof and abs(v - w) < 1e-3 for d, w in cases):
                cases.append((dof, v))
    for k in range(pk.npathpt):
        pt = pk.pathpt[k]
        if pt.type == 1:
            add(pt.cond_coord, pt.range_lo, pt.range_hi)
        if pt.type == 2:
            for a in range(3):
                if pt.fn[a] >= 0:
                    fn = pk.fn[pt.fn[a]]
                    if fn.type == 2:
                        add(fn.coord, pk.knot_x[fn.knot_off], pk.knot_x[fn.knot_off + fn.nknots - 1])
    return cases


@pytest.mark.parametrize('env_id', [M2D, MLK2D])
def test_conditional_and_moving_points_on_both_sides(env_id):
    """one env per case on a mid-table reset state, each with one coordinate that a
    conditional or moving path point depends on placed below, inside or above
    the point's range (set_state); one step against the oracle from the same
    states"""
    import torch
    from bioimitation.registry import load_pack
    cases = _point_cases(load_pack(env_id))
    n = len(cases)
    assert 6 <= n <= 48, cases
    pk, orc, bufs = _oracle(env_id, n)
    env = _env(env_id, n)
    rows = np.full(n, pk.reset_hi // 2, dtype=np.int32)
    env.reset(ref_index=rows)
    state = env.get_state()
    for i in range(n):
        dof, v = cases[i % len(cases)]
        state[i, 5 + dof] = v
        state[i, 5 + pk.ndof + dof] = 0.3 * (-1) ** i
    env.set_state(state)
    for i in range(n):
        orc.reset(bufs, i, int(rows[i]))
        orc.set_state(bufs, i, state[i])
    acts = _actions(pk, np.random.default_rng(6), rows)
    obs, rew, done, info = env.step(torch.as_tensor(acts, device=env.device))
    torch.cuda.synchronize()
    obs, rew, done, info = (x.cpu().numpy() for x in (obs, rew, done, info))
    worst = 0.0
    for i in range(n):
        o, r, d, inf = orc.step(bufs, i, acts[i])
        e = max(_rel(obs[i], o).max(), abs(rew[i] - r), _rel(info[i], inf).max())
        print(f'{env_id} env {i}: dof {cases[i % len(cases)][0]} at {cases[i % len(cases)][1]:+.3f}, err {e:.2e}')
        assert bool(done[i]) == d, i
        assert e < TOL, (i, cases[i % len(cases)], e)
        worst = max(worst, e)
    print(f'{env_id}: {len(cases)} point cases, max rel err {worst:.2e}')
    env.close()


def test_record_belongs_to_the_launch():
    """two handles of different packs on one compiled topology (the planar
    muscle walking and running models), stepped alternately in one process:
    each gives, bit for bit, what a handle of its pack gives stepped alone"""
    import torch
    from bioimitation.registry import load_pack
    n, steps = 16, 6
    out = {}
    for mode in ('alternate', 'alone'):
        envs = {k: _env(k, n) for k in (M2D, MR2D)} if mode == 'alternate' else {}
        got = {M2D: [], MR2D: []}
        acts, rows = {}, {}
        for k in (M2D, MR2D):
            pk = load_pack(k)
            rows[k] = np.array([(3 + 5 * i) % (pk.reset_hi + 1) for i in range(n)], dtype=np.int32)
            acts[k] = np.random.default_rng(9).uniform(0.0, 1.0, size=(steps, n, pk.nact))
        if mode == 'alternate':
            for k in (M2D, MR2D):
                envs[k].reset(ref_index=rows[k])
            for t in range(steps):
                for k in (M2D, MR2D):
                    got[k].append(_cat(envs[k].step(torch.as_tensor(acts[k][t], device=envs[k].device))))
        else:
            for k in (M2D, MR2D):
                envs[k] = _env(k, n)
                envs[k].reset(ref_index=rows[k])
                for t in range(steps):
                    got[k].append(_cat(envs[k].step(torch.as_tensor(acts[k][t], device=envs[k].device))))
        torch.cuda.synchronize()
        out[mode] = {k: torch.stack(v).cpu() for k, v in got.items()}
        for e in envs.values():
            e.close()
    assert not torch.equal(out['alone'][M2D], out['alone'][MR2D])   # the packs differ
    for k in (M2D, MR2D):
        assert torch.equal(out['alternate'][k], out['alone'][k]), k


def test_fused_rollout_equals_single_steps():
    """a 4-step fused rollout of 16 planar muscle envs against 4 single steps
    with the same actions, bit for bit: the record is right at every step of
    the launch (a rollout step runs the single step's prologue, which stages the
    image and builds the record again)"""
    import torch
    from bioimitation.registry import load_pack
    n, steps = 16, 4
    pk = load_pack(M2D)
    rows = np.array([pk.reset_hi // 2 + i for i in range(n)], dtype=np.int32)
    a, b = _env(M2D, n), _env(M2D, n)
    acts = torch.as_tensor(np.random.default_rng(10).uniform(0.0, 1.0, size=(steps, n, pk.nact)), device=a.device).contiguous()
    a.reset(ref_index=rows)
    b.reset(ref_index=rows)
    ro, rr, rd, ri = a.rollout(acts, obs='all', info=True)
    assert a.last_rollout_fused
    single = [tuple(x.clone() for x in b.step(acts[t])) for t in range(steps)]
    torch.cuda.synchronize()
    for t in range(steps):
        o, r, d, inf = single[t]
        assert torch.equal(ro[t], o) and torch.equal(rr[t], r) and torch.equal(ri[t], inf), t
        assert torch.equal(rd[t].to(torch.bool), d.to(torch.bool)), t
    assert np.array_equal(a.get_state(), b.get_state())
    a.close()
    b.close()


def test_other_kernels_between_steps():
    """step, an inverse-dynamics call and a muscle analysis on the same
    handle, step: bitwise the two steps of a handle that ran nothing in
    between (the record is rebuilt by each launch; the analysis kernels only
    read the envs)"""
    import torch
    from bioimitation import inverse_dynamics as idyn
    from bioimitation._analysis import ptr
    from bioimitation import _lib
    from bioimitation.registry import load_pack
    n = 16
    pk = load_pack(M2D)
    rows = np.array([pk.reset_hi // 3 + 2 * i for i in range(n)], dtype=np.int32)
    a, b = _env(M2D, n), _env(M2D, n)
    acts = torch.as_tensor(np.random.default_rng(11).uniform(0.0, 1.0, size=(2, n, pk.nact)), device=a.device).contiguous()
    a.reset(ref_index=rows)
    b.reset(ref_index=rows)
    got, want = [_cat(a.step(acts[0]))], [_cat(b.step(acts[0]))]
    q = torch.as_tensor(a.get_state()[:, 5:5 + pk.ndof], device=a.device).contiguous()
    out = torch.empty_like(q)
    _lib.check(a._L.bioim_id_eval(a._h, idyn.TOTAL, n, ptr(q), ptr(torch.zeros_like(q)), None, ptr(out)))
    ma = a.muscle_analysis()
    assert torch.isfinite(out).all() and all(torch.isfinite(v).all() for v in ma.values())
    got.append(_cat(a.step(acts[1])))
    want.append(_cat(b.step(acts[1])))
    torch.cuda.synchronize()
    for k, (x, y) in enumerate(zip(got, want)):
        assert torch.equal(x, y), k
    assert np.array_equal(a.get_state(), b.get_state())
    a.close()
    b.close()
