"""The step launch around its dynamics calls: the substep update formed
inside the call, q'' published by the realize only, the ground slot's
constants written once per launch and again before a reset realize that
follows a report, and the report's reference rows at the end of the table
(csrc/bioim_step.hip: env_block, dynamics).

Shapes: 1, 17 and 40 envs at 16 envs per workgroup are one lane group of one
wave, a second workgroup that holds a single env, and a partly filled last
workgroup.  IDs: the planar muscle model, the planar torque model (PD
pre-pass, torque cache, the reset table's torque rows) and the spatial running
model (two muscles per lane).

Every run is STEPS steps with auto-reset on and starts near the end of the
reference table: env i starts at one of START (relative to the pack), so some
envs step over istep >= n_episode (terminated, reset in the launch, then step
on from the drawn row) and some report from the last reference row, where the
target observation's row istep + 1 is clamped to it.  Both are asserted.

Against the oracle: observation (the pre-reset one through final_obs, and the
reset's own against the oracle reset at the drawn row), reward, done and info
of every env and step, at test_gpu_parity's fp64 free-running bound (1e-6 of
max(|x|, 1); reward absolute).  Self-consistency is bitwise (one documented
exception in test_reset_table_on_equals_off)."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason='needs a HIP GPU')]

M2D, T2D, R3D = 'MuscleWalkingImitation2D-v0', 'TorqueWalkingImitation2D-v0', 'MuscleRunningImitation3D-v0'
IDS = [M2D, T2D, R3D]
SIZES = [1, 17, 40]
STEPS = 10
SEED = 13
TOL = 1e-6


def _start_rows(pk, n):
    """env i: the row before the last one (its first report reads the clamped
    row istep + 1 = nrows, and istep >= n_episode ends it), 3 and 2 steps
    before the episode limit, and a mid-table row that just keeps stepping"""
    start = [pk.nrows - 2, pk.n_episode - 3, pk.n_episode - 2, pk.reset_hi // 2]
    return np.array([start[i % len(start)] for i in range(n)], dtype=np.int32)


def _actions(pk, rng, isteps):
    """muscle excitations U[0, 1]; torque models: PD targets of the next
    reference row + N(0, 0.05) (test_gpu_parity's drive)"""
    n = len(isteps)
    if pk.nmuscle:
        return rng.uniform(0.0, 1.0, size=(n, pk.nact))
    base = np.array([[pk.ref_q[min(int(r) + 1, pk.nrows - 1)][pk.pd_coord[a]] for a in range(pk.nact)] for r in isteps])
    return base + rng.normal(0.0, 0.05, size=(n, pk.nact))


def _action_seq(pk, rows, steps=STEPS, seed=3):
    """(steps, n, A) actions that do not depend on the run (the torque drive
    follows the start row + t, wherever a reset has put the env since)"""
    rng = np.random.default_rng(seed)
    return np.stack([_actions(pk, rng, rows + t) for t in range(steps)])


def _rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def _env(env_id, n, config=None, env_offset=0, reset_table=True):
    from bioimitation.vector_env import VectorEnv
    env = VectorEnv(env_id, n, config=config, precision=64, seed=SEED, auto_reset=True, env_offset=env_offset)
    env.set_reset_table(reset_table)
    return env


def _oracle_run(env_id, n, config=None):
    """STEPS auto-reset steps on the GPU against the oracle, env by env"""
    import torch
    import oracle
    from bioimitation.registry import load_pack
    pk = load_pack(env_id, config)
    env = _env(env_id, n, config)
    env.enable_final_obs()
    orc = oracle.Oracle(pk)
    bufs = orc.new_envs(n)
    rows = _start_rows(pk, n)
    acts = _action_seq(pk, rows)
    obs0 = env.reset(ref_index=rows).cpu().numpy()
    for i in range(n):
        assert _rel(obs0[i], orc.reset(bufs, i, int(rows[i]))).max() < TOL, i
    ref_istep = np.array(pk.ref_istep[:pk.nrows])
    worst, terminated, clamped, limit_ended = 0.0, 0, 0, 0
    for t in range(STEPS):
        obs, rew, done, info = env.step(torch.as_tensor(acts[t], device=env.device))
        torch.cuda.synchronize()
        obs, rew, done, info, fin = (x.cpu().numpy() for x in (obs, rew, done, info, env.final_obs))
        state = env.get_state()
        for i in range(n):
            o, r, d, inf = orc.step(bufs, i, acts[t, i])
            istep = int(orc.get_state(bufs, i)[1])          # the step's own report, before any reset
            clamped += int(istep + 1 >= pk.nrows)
            limit_ended += int(d and istep >= pk.n_episode)
            e = max(_rel(fin[i], o).max(), abs(rew[i] - r), _rel(info[i], inf).max())
            print(f'{env_id} n={n} t={t} env {i}: istep {istep} done {d} err {e:.2e}')
            assert e < TOL, (t, i, e)
            assert bool(done[i]) == d, (t, i)
            worst = max(worst, e)
            if not d:
                assert np.array_equal(obs[i], fin[i]), (t, i)
                continue
            # reset in the launch: the row it drew is the one of the state's istep whose oracle
            # reset gives the launch's observation
            terminated += 1
            cand = [int(c) for c in np.where(ref_istep[:pk.reset_hi + 1] == int(state[i, 1]))[0]]
            errs = [_rel(obs[i], orc.reset(bufs, i, c)).max() for c in cand]
            assert cand and min(errs) < TOL, (t, i, state[i, 1], cand, errs)
            orc.reset(bufs, i, cand[int(np.argmin(errs))])
            worst = max(worst, min(errs))
    print(f'{env_id} n={n} {config}: {STEPS} steps, max rel err {worst:.2e}, {terminated} terminations '
          f'({limit_ended} at the episode limit), {clamped} reports on the clamped row')
    assert terminated >= 1 and limit_ended >= 1, (terminated, limit_ended)
    assert clamped >= 1, clamped
    env.close()


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('env_id', IDS)
def test_step_tail_vs_oracle(env_id, n):
    _oracle_run(env_id, n)


@pytest.mark.parametrize('config', [{'use_target_obs': False}, {'use_GRF': False}])
def test_step_tail_vs_oracle_obs_switches(config):
    """without the target observation (no row istep + 1 is read) and without
    the ground reaction forces, on the planar muscle model in two workgroups"""
    _oracle_run(M2D, 17, config)


def _run(env, rows, acts):
    """reset to rows, then step through acts: every output of every step, and the end state"""
    import torch
    out = [env.reset(ref_index=rows).clone()]
    for t in range(acts.shape[0]):
        o, r, d, inf = env.step(acts[t])
        out.append(torch.cat([o, r[:, None], d[:, None].to(o.dtype), inf], 1).clone())
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out], env.get_state()


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('env_id', IDS)
def test_reset_table_on_equals_off(env_id, n):
    """an auto-reset from the reset table (no realize in the launch) and one
    that runs the reset realize after the report give the same bits: every
    step's observation, reward, done and info and the end state.  One part is
    not bitwise by the table's construction (DESIGN.md 5.7, and
    test_gpu_parity.test_reset_table_matches_reset_realize): a torque model's
    table row forms the reset observation's q'' as q''(0) + M^-1 tau with the
    inverse-dynamics kernel's M, the realize by its own factorization, so
    those columns of a reset row are held to that test's 1e-10 instead
    (measured 4e-12 there)."""
    import torch
    from bioimitation.registry import load_pack
    pk = load_pack(env_id)
    rows = _start_rows(pk, n)
    runs = []
    for table in (True, False):
        env = _env(env_id, n, reset_table=table)
        acts = torch.as_tensor(_action_seq(pk, rows), device=env.device)
        runs.append(_run(env, rows, acts))
        if table:
            assert env.reset_table_rows > 0
        env.close()
    (a, sa), (b, sb) = runs
    assert any(x[:, pk.obs_dim + 1].any() for x in a[1:])        # a reset ran in a launch
    ntrans = sum(1 for c in (pk.coord_tx, pk.coord_ty, pk.coord_tz) if c >= 0)
    qdd0 = 1 + (pk.ncoord - ntrans) + pk.ncoord
    for t, (x, y) in enumerate(zip(a, b)):
        exact = np.ones(x.shape, bool)
        if not pk.nmuscle and t > 0:
            exact[np.ix_(x[:, pk.obs_dim + 1] != 0, np.arange(qdd0, qdd0 + pk.ncoord))] = False
        assert np.array_equal(x[exact], y[exact]), t
        assert (_rel(x[~exact], y[~exact]) < 1e-10).all(), t
    assert np.array_equal(sa, sb)


@pytest.mark.parametrize('env_id', IDS)
def test_env_alone_equals_its_batch_slot(env_id):
    """an env stepped alone (one lane group, env offset k) against the same env
    at slot k of the 40-env batch: the last slot of a full workgroup, the first
    of the next one and the last of the partly filled one"""
    import torch
    from bioimitation.registry import load_pack
    pk = load_pack(env_id)
    n = 40
    rows = _start_rows(pk, n)
    seq = _action_seq(pk, rows)
    batch = _env(env_id, n)
    full, sfull = _run(batch, rows, torch.as_tensor(seq, device=batch.device))
    batch.close()
    for k in (15, 16, 39):
        one = _env(env_id, 1, env_offset=k)
        alone, sone = _run(one, rows[k:k + 1], torch.as_tensor(seq[:, k:k + 1], device=one.device).contiguous())
        one.close()
        for t, (x, y) in enumerate(zip(alone, full)):
            assert np.array_equal(x[0], y[k]), (k, t)
        assert np.array_equal(sone[0], sfull[k]), k


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('env_id', IDS)
def test_rollout_of_3_equals_3_steps(env_id, n):
    """one rollout launch over 3 steps (the env block run three times in one
    kernel: the ground slot's constants are written by each) against three
    step launches, from the start rows, so the rollout holds the terminations"""
    import torch
    from bioimitation.registry import load_pack
    pk = load_pack(env_id)
    rows = _start_rows(pk, n)
    a, b = _env(env_id, n), _env(env_id, n)
    acts = torch.as_tensor(_action_seq(pk, rows, steps=3), device=a.device).contiguous()
    a.reset(ref_index=rows)
    b.reset(ref_index=rows)
    obs, rew, done, info = a.rollout(acts, obs='all', info=True)
    assert a.last_rollout_fused
    for t in range(3):
        o, r, d, inf = b.step(acts[t])
        assert torch.equal(obs[t], o) and torch.equal(rew[t], r) and torch.equal(done[t], d) and torch.equal(info[t], inf), t
    assert bool(done.any())
    assert np.array_equal(a.get_state(), b.get_state())
    a.close()
    b.close()
