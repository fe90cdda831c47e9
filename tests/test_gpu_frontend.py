"""The kinematics front end of the step kernels' dynamics call
(csrc/bioim_kinematics.h, BIOIM_FRONTEND: joint columns summed in registers,
branch-free axis kinds in the planar joint-local kinematics, the chain's frame
handed to the inertias in registers, the first chain level composed from the
ground frame), and the force elements that read what it publishes (the
coordinate limits in every regime).

Shapes: 1, 17 and 40 envs at 16 envs per workgroup are one lane group, a
second workgroup that holds one env, and a partly filled last workgroup.
IDs: the planar muscle and torque models, the planar locked-knee muscle model
(coordinates without a dof: axes that move no column, constant published
values) and the spatial running model (a body with six dofs, two muscle
passes).

Bounds: a stepped state against the oracle at test_gpu_parity's fp64
free-running bound (1e-6 of max(|x|, 1); reward absolute); a realized state
that was not stepped (a reset) at the suite's 5e-9; self-consistency bitwise."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason='needs a HIP GPU')]

M2D, T2D = 'MuscleWalkingImitation2D-v0', 'TorqueWalkingImitation2D-v0'
LK2D, R3D = 'MuscleLockedKneeImitation2D-v0', 'MuscleRunningImitation3D-v0'
IDS = [M2D, T2D, LK2D, R3D]
SIZES = [1, 17, 40]
STEPS = 10
SEED = 13
TOL, TOL_REALIZE = 1e-6, 5e-9


def _rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def _start_rows(pk, n):
    """test_gpu_step_tail's: the row before the last, 3 and 2 steps before the
    episode limit, and a mid-table row"""
    start = [pk.nrows - 2, pk.n_episode - 3, pk.n_episode - 2, pk.reset_hi // 2]
    return np.array([start[i % len(start)] for i in range(n)], dtype=np.int32)


def _actions(pk, rng, isteps):
    """test_gpu_step_tail's drives: muscle excitations U[0, 1]; torque models:
    PD targets of the next reference row + N(0, 0.05)"""
    n = len(isteps)
    if pk.nmuscle:
        return rng.uniform(0.0, 1.0, size=(n, pk.nact))
    base = np.array([[pk.ref_q[min(int(r) + 1, pk.nrows - 1)][pk.pd_coord[a]] for a in range(pk.nact)] for r in isteps])
    return base + rng.normal(0.0, 0.05, size=(n, pk.nact))


def _action_seq(pk, rows, steps=STEPS, seed=3):
    rng = np.random.default_rng(seed)
    return np.stack([_actions(pk, rng, rows + t) for t in range(steps)])


def _env(env_id, n, auto_reset=True):
    from bioimitation.vector_env import VectorEnv
    return VectorEnv(env_id, n, precision=64, seed=SEED, auto_reset=auto_reset)


def _oracle(env_id, n):
    import oracle
    from bioimitation.registry import load_pack
    pk = load_pack(env_id)
    orc = oracle.Oracle(pk)
    return pk, orc, orc.new_envs(n)


def _columns(env_id, pk, prefixes):
    from bioimitation.obslayout import column_names, load_names
    names = column_names(pk, load_names(env_id))
    return np.array([i for i, c in enumerate(names) if c.startswith(prefixes)])


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('env_id', IDS)
def test_free_running_parity(env_id, n):
    """ten auto-reset steps against the oracle: observation (the step's own,
    through final_obs, and a reset's against the oracle reset at the row the
    launch drew), reward, done and info of every env and step"""
    import torch
    pk, orc, bufs = _oracle(env_id, n)
    env = _env(env_id, n)
    env.enable_final_obs()
    rows = _start_rows(pk, n)
    acts = _action_seq(pk, rows)
    obs0 = env.reset(ref_index=rows).cpu().numpy()
    for i in range(n):
        assert _rel(obs0[i], orc.reset(bufs, i, int(rows[i]))).max() < TOL, i
    ref_istep = np.array(pk.ref_istep[:pk.nrows])
    worst, resets = 0.0, 0
    for t in range(STEPS):
        obs, rew, done, info = env.step(torch.as_tensor(acts[t], device=env.device))
        torch.cuda.synchronize()
        obs, rew, done, info, fin = (x.cpu().numpy() for x in (obs, rew, done, info, env.final_obs))
        state = env.get_state()
        for i in range(n):
            o, r, d, inf = orc.step(bufs, i, acts[t, i])
            e = max(_rel(fin[i], o).max(), abs(rew[i] - r), _rel(info[i], inf).max())
            assert e < TOL, (t, i, e)
            assert bool(done[i]) == d, (t, i)
            worst = max(worst, e)
            if not d:
                assert np.array_equal(obs[i], fin[i]), (t, i)
                continue
            resets += 1
            cand = [int(c) for c in np.where(ref_istep[:pk.reset_hi + 1] == int(state[i, 1]))[0]]
            errs = [_rel(obs[i], orc.reset(bufs, i, c)).max() for c in cand]
            assert cand and min(errs) < TOL, (t, i, state[i, 1], cand, errs)
            orc.reset(bufs, i, cand[int(np.argmin(errs))])
    print(f'{env_id} n={n}: {STEPS} steps, max rel err {worst:.2e}, {resets} resets in a launch')
    assert resets >= 1
    env.close()


@pytest.mark.parametrize('env_id', IDS)
def test_reset_realize(env_id):
    """the reset's realize at the first row, a middle row and the last valid
    row: q'' and the body-position blocks of the observation"""
    n = 40
    pk, orc, bufs = _oracle(env_id, n)
    env = _env(env_id, n)
    pick = [0, pk.reset_hi // 2, pk.reset_hi]
    rows = np.array([pick[i % 3] for i in range(n)], dtype=np.int32)
    obs = env.reset(ref_index=rows).cpu().numpy()
    ref = np.stack([orc.reset(bufs, i, int(rows[i])) for i in range(n)])
    cols = _columns(env_id, pk, ('coordinate_acc', 'body_pos'))
    assert len(cols) >= pk.ncoord + 3
    e = _rel(obs[:, cols], ref[:, cols])
    print(f'{env_id}: reset realize, rows {pick}, max rel err {e.max():.2e}')
    assert e.max() < TOL_REALIZE, (e.max(), np.unravel_index(e.argmax(), e.shape))
    env.close()


REGIMES = ['inside', 'lower transition', 'upper transition', 'below', 'above']


def _regime_value(lm, regime):
    """a coordinate value in the limit force's regime: the range is
    [qlow, qup], each end has a transition zone of width trans outside it"""
    return {'inside': 0.5 * (lm.qlow + lm.qup), 'lower transition': lm.qlow - 0.5 * lm.trans,
            'upper transition': lm.qup + 0.5 * lm.trans, 'below': lm.qlow - 1.5 * lm.trans,
            'above': lm.qup + 1.5 * lm.trans}[regime]


@pytest.mark.parametrize('env_id', IDS)
def test_limit_regimes(env_id):
    """one env per coordinate limit and regime (inside the range, inside either
    transition, beyond either end), placed with set_state on a mid-table reset
    state with the coordinate moving at 0.5 / s; one step with the force
    report on: the limit rows and the observation"""
    import torch
    from bioimitation.registry import load_pack
    pk0 = load_pack(env_id)
    cases = [(li, rg) for li in range(pk0.nlimit) if pk0.limit[li].dof >= 0 for rg in REGIMES]
    n = len(cases)
    assert n >= len(REGIMES)
    pk, orc, bufs = _oracle(env_id, n)
    env = _env(env_id, n, auto_reset=False)
    env.enable_force_report()
    rows = np.full(n, pk.reset_hi // 2, dtype=np.int32)
    env.reset(ref_index=rows)
    state = env.get_state()
    nd = pk.ndof
    for i, (li, rg) in enumerate(cases):
        lm = pk.limit[li]
        state[i, 5 + lm.dof] = _regime_value(lm, rg)
        state[i, 5 + nd + lm.dof] = 0.5
    env.set_state(state)
    for i in range(n):
        orc.reset(bufs, i, int(rows[i]))
        orc.set_state(bufs, i, state[i])
    acts = _actions(pk, np.random.default_rng(5), rows)
    obs, rew, done, info = env.step(torch.as_tensor(acts, device=env.device))
    torch.cuda.synchronize()
    obs, rep = obs.cpu().numpy(), env.force_report.cpu().numpy()
    l0 = pk.nact + 6 * pk.ncforce
    worst = 0.0
    for i, (li, rg) in enumerate(cases):
        o = orc.step(bufs, i, acts[i])[0]
        want = orc.force_report(bufs, i)[l0:l0 + pk.nlimit]
        e = max(_rel(rep[i, l0:l0 + pk.nlimit], want).max(), _rel(obs[i], o).max())
        print(f'{env_id} limit {li} {rg}: limit rows {want}, err {e:.2e}')
        assert e < TOL, (li, rg, e)
        worst = max(worst, e)
    print(f'{env_id}: {n} limit cases, max rel err {worst:.2e}')
    env.close()


@pytest.mark.parametrize('env_id', IDS)
def test_step_outputs_survive_other_kernels(env_id):
    """one handle runs step, reset, step, body_kinematics, inverse_dynamics,
    get_state / set_state, a 3-step rollout, step; its step and rollout outputs
    are bitwise those of a handle that ran only the steps and the rollout from
    the same states (set_state puts it where the first one's reset went; both
    handles pass through set_state at the same points, so each launch starts
    with or without the realize cache in both)"""
    import torch
    from bioimitation import inverse_dynamics as idyn
    from bioimitation._analysis import ptr
    from bioimitation import _lib
    from bioimitation.registry import load_pack
    n = 17
    pk = load_pack(env_id)
    # mid-table rows: no env ends in these 6 steps (asserted), since the row an auto-reset draws
    # depends on the handle's reset count, which the first handle's own reset advances
    mid = [pk.reset_hi // 2, pk.reset_hi // 3, pk.reset_hi // 4, 5]
    rows = np.array([mid[i % len(mid)] for i in range(n)], dtype=np.int32)
    a, b = _env(env_id, n), _env(env_id, n)
    acts = torch.as_tensor(_action_seq(pk, rows, steps=6), device=a.device).contiguous()

    def cat(out):
        o, r, d, inf = out
        return torch.cat([o, r[:, None], d[:, None].to(o.dtype), inf], 1).clone()

    a.reset(ref_index=rows)
    b.reset(ref_index=rows)
    got, want = [cat(a.step(acts[0]))], [cat(b.step(acts[0]))]
    a.reset(ref_index=rows[::-1].copy())
    s = a.get_state()
    a.set_state(s)
    b.set_state(s)
    got.append(cat(a.step(acts[1])))
    want.append(cat(b.step(acts[1])))
    a.body_kinematics()
    q = torch.as_tensor(a.get_state()[:, 5:5 + pk.ndof], device=a.device).contiguous()
    out = torch.empty_like(q)
    _lib.check(a._L.bioim_id_eval(a._h, idyn.TOTAL, n, ptr(q), ptr(torch.zeros_like(q)), None, ptr(out)))
    a.set_state(a.get_state())
    b.set_state(b.get_state())
    ra = a.rollout(acts[2:5], obs='all', info=True)
    rb = b.rollout(acts[2:5], obs='all', info=True)
    assert a.last_rollout_fused and b.last_rollout_fused
    got.append(cat(a.step(acts[5])))
    want.append(cat(b.step(acts[5])))
    torch.cuda.synchronize()
    assert not any(bool(y[:, pk.obs_dim + 1].any()) for y in want) and not bool(rb[2].any())
    for k, (x, y) in enumerate(zip(got, want)):
        assert torch.equal(x, y), k
    for k, (x, y) in enumerate(zip(ra, rb)):
        assert torch.equal(x, y), k
    assert np.array_equal(a.get_state(), b.get_state())
    a.close()
    b.close()
