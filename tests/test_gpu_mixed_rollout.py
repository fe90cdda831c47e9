"""Group rollouts and per-env state calls of the mixed batch:
``MixedVectorEnv.rollout`` over bioim_rollout_group — T steps of a
two-topology batch in one launch of rollout_kernel2 where the group step
fuses, T group steps from C otherwise — and the global-id reset, mask and
state calls.  fp64; every comparison is bitwise against a twin
``MixedVectorEnv`` of the same seed that is stepped.

21 LockedKnee3D + 13 Palsy3D envs at 16 envs per workgroup: segment 0 is one
full workgroup and a partial one of 5, segment 1 starts at global env 21 (no
multiple of 16) in a partial workgroup of its own, so a wrong block offset,
row offset or sequence pitch shows.  T_ROLL = 32 after 3 warm steps ends at
step 34 from reset: under this drive the fp64 CPU oracle has LockedKnee3D's
first dones at steps 24, 26, 27, 29 (9 of 21 envs never done in 60 steps) and
Palsy3D's at 24, 24, 24, 25, 27, 27, 28, 33, 34 (4 of 13 not done by step
34), so each segment has a done before the last step and an env that is never
done.  Both are asserted; the tests print their done counts.  On the GPU the
first dones fall in rollout steps 21, 23, 24, 26 (LockedKnee3D) and 21, 21,
21, 22, 24, 24, 25, 30 (Palsy3D), the oracle's steps less the 3 warm ones, so
T_ROLL = 32 stands."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason='needs a HIP GPU')]

LK3D, P3D = 'MuscleLockedKneeImitation3D-v0', 'MusclePalsyImitation3D-v0'
M2D, T2D, R3D = 'MuscleWalkingImitation2D-v0', 'TorqueWalkingImitation2D-v0', 'MuscleRunningImitation3D-v0'
SEGS = [(LK3D, 21), (P3D, 13)]
SEGS3 = [(M2D, 5), (T2D, 4), (R3D, 3)]
WARM = 3            # ordinary steps first: the rollout starts from a valid realize cache
T_ROLL = 32
T_MAX = 60          # actions are always drawn for T_MAX steps, so a prefix does not depend on T
PLANES = ('cache', 'cache_ok', 'vnw', 'resets')
SENTINEL = -7.25


def _drive(env_id, n):
    """per segment, from a fresh default_rng(201): reference rows (one per
    env) and (T_MAX, n, A) actions — muscle models U[0, 0.4], torque models
    the PD targets of the next reference row + N(0, 0.05)"""
    from bioimitation.registry import load_pack
    pk = load_pack(env_id)
    rng = np.random.default_rng(201)
    rows = rng.integers(0, min(pk.reset_hi, pk.nrows - T_MAX - 2) + 1, size=n).astype(np.int32)
    if pk.nmuscle:
        acts = rng.uniform(0.0, 0.4, size=(T_MAX, n, pk.nact))
    else:
        acts = np.stack([np.array([[pk.ref_q[min(int(r) + t + 1, pk.nrows - 1)][pk.pd_coord[a]] for a in range(pk.nact)]
                                   for r in rows]) for t in range(T_MAX)]) + rng.normal(0.0, 0.05, size=(T_MAX, n, pk.nact))
    return rows, acts


def _pair(segs, auto_reset=True, config=None, warm=WARM):
    """two mixed batches of the same seed at the same state, `warm` steps in,
    and the remaining padded actions on the device, (T_MAX - warm, N, max A)"""
    import torch
    from bioimitation.vector_env import MixedVectorEnv
    envs = [MixedVectorEnv(segs, config=config, precision=64, seed=5, auto_reset=auto_reset) for _ in range(2)]
    m = envs[0]
    acts = np.zeros((T_MAX, m.num_envs, m.action_dim))
    rows = []
    for (env_id, n), off, e in zip(segs, m.offsets, m.envs):
        r, a = _drive(env_id, n)
        rows.append(r)
        acts[:, off:off + n, :e.action_dim] = a
    dev = torch.as_tensor(acts, device=m.device, dtype=m.dtype).contiguous()
    for m in envs:
        for e, r in zip(m.envs, rows):
            e.reset(ref_index=r)
        for t in range(warm):
            m.step(dev[t])
    return envs[0], envs[1], dev[warm:]


def _stepped(env, acts, want_state=False):
    """T step() calls, every output cloned: (obs, reward, done, info[, state rows]) as (T, N, ...) arrays"""
    import torch
    seq = [[], [], [], [], []]
    for t in range(acts.shape[0]):
        out = env.step(acts[t])
        for k in range(4):
            seq[k].append(out[k].clone())
        if want_state:
            seq[4].append(env.state_rows())
    torch.cuda.synchronize()
    return tuple(torch.stack(s).cpu().numpy() for s in seq[:5 if want_state else 4])


def _np(*ts):
    import torch
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def _slices(m):
    return [slice(off, off + e.num_envs) for off, e in zip(m.offsets, m.envs)]


def _assert_same_envs(a, b):
    """state, debug planes and reset counters of every segment"""
    for ea, eb in zip(a.envs, b.envs):
        assert np.array_equal(ea.get_state(), eb.get_state()), ea.env_id
        for name in PLANES:
            assert np.array_equal(ea.debug_plane(name), eb.debug_plane(name)), (ea.env_id, name)
        assert ea.reset_count() == eb.reset_count()


def _fusion(on):
    from bioimitation import _lib
    _lib.load().bioim_set_group_fusion(1 if on else 0)


@pytest.mark.parametrize('fusion', [1, 0])
def test_group_rollout_is_bit_identical_to_group_stepping(fusion):
    """Auto-reset on; the rollout is issued as two calls (T - 5 and 5 steps),
    so the second starts from the state, realize cache and reset counters the
    first left.  fusion 1: one launch of rollout_kernel2 per call (the C5
    order, LockedKnee3D first, runs the <Walking3D, LockedKnee3D>
    instantiation with the argument sets swapped); fusion 0: the host loop
    over forked per-segment launches."""
    import torch
    _fusion(fusion)
    try:
        a, b, acts = _pair(SEGS)
        assert all(e.launch['envs_per_workgroup'] == 16 for e in a.envs)
        assert a.offsets == [0, 21] and tuple(acts.shape[1:]) == (34, a.action_dim)
        T = T_ROLL
        first = a.rollout(acts[:T - 5], obs='all', info=True)
        assert a.last_rollout_fused == bool(fusion)
        second = a.rollout(acts[T - 5:T], obs='all', info=True)
        assert a.last_rollout_fused == bool(fusion)
        ro, rr, rd, ri = _np(*(torch.cat([x, y]) for x, y in zip(first, second)))
        so, sr, sd, si = _stepped(b, acts[:T])
        assert b.last_step_fused == bool(fusion)
        assert rd.shape == (T, 34) and rd.dtype == np.uint8 and ro.shape == (T, 34, a.obs_dim)
        for e, sl in zip(a.envs, _slices(a)):
            d = sd[:, sl]
            ever = d.any(axis=0)
            print(f'{e.env_id} fusion={fusion}: {int(d.sum())} dones in {T} steps, first at step '
                  f'{int(np.argmax(d.any(axis=1)))}, {int(ever.sum())}/{e.num_envs} envs were done, '
                  f'{int(d[:-1].sum())} before the last step')
        assert np.array_equal(rr, sr)
        assert np.array_equal(rd, sd)
        assert np.array_equal(ro, so)
        assert np.array_equal(ri, si)
        assert np.array_equal(a.obs.cpu().numpy(), b.obs.cpu().numpy())     # obs='all' leaves the last rows in self.obs too
        _assert_same_envs(a, b)
        for e, sl in zip(a.envs, _slices(a)):      # buffers the call allocated: zero padding columns
            assert not ro[:, sl, e.obs_dim:].any() and not ri[:, sl, e.info_dim:].any()
            d = sd[:, sl]
            # conditions, not skips: each segment ran the in-loop auto-reset and kept an env going throughout
            assert d[:-1].any(), f'{e.env_id}: no env was done before the last step'
            assert not d.any(axis=0).all(), f'{e.env_id}: every env was done'
        a.close(), b.close()
    finally:
        _fusion(1)


def test_group_rollout_host_loop_for_a_pair_without_a_fused_kernel():
    """three segments (planar muscle, planar torque, spatial running): no
    fused kernel, so the call loops over the forked per-segment launches"""
    a, b, acts = _pair(SEGS3)
    T = 6
    ro, rr, rd, ri = _np(*a.rollout(acts[:T], obs='all', info=True))
    assert not a.last_rollout_fused
    so, sr, sd, si = _stepped(b, acts[:T])
    assert np.array_equal(rr, sr) and np.array_equal(rd, sd) and np.array_equal(ro, so) and np.array_equal(ri, si)
    assert np.array_equal(a.obs.cpu().numpy(), b.obs.cpu().numpy())
    _assert_same_envs(a, b)
    a.close(), b.close()


@pytest.mark.parametrize('fusion', [1, 0])
def test_group_stop_at_done_and_active_mask(fusion):
    """Auto-reset off; global envs 0, 20 and 21 (the segment boundary) are
    masked out and their rows prefilled with a sentinel.  A live env is
    stepped until its first done; later rows are reward 0, done 1, info 0
    and the terminal observation again."""
    import torch
    _fusion(fusion)
    try:
        a, b, acts = _pair(SEGS, auto_reset=False)
        n, T = a.num_envs, T_ROLL
        masked = [0, 20, 21]
        mask = torch.ones(n, dtype=torch.uint8, device=a.device)
        mask[masked] = 0
        keep = mask.clone()
        a.set_active_mask(mask)
        b.set_active_mask(mask)
        before = a.state_rows().cpu().numpy()
        obs_before = a.obs.cpu().numpy().copy()
        out = {'reward': torch.full((T, n), SENTINEL, dtype=a.dtype, device=a.device),
               'done': torch.full((T, n), 9, dtype=torch.uint8, device=a.device),
               'obs': torch.full((T, n, a.obs_dim), SENTINEL, dtype=a.dtype, device=a.device),
               'info': torch.full((T, n, a.info_dim), SENTINEL, dtype=a.dtype, device=a.device)}
        res = a.rollout(acts[:T], obs='all', info=True, stop_at_done=True, out=out)
        assert a.last_rollout_fused == bool(fusion)
        assert res[0] is out['obs'] and res[1] is out['reward'] and res[2] is out['done'] and res[3] is out['info']
        ro, rr, rd, ri = _np(*res)
        so, sr, sd, si, ss = _stepped(b, acts[:T], want_state=True)
        after = a.state_rows().cpu().numpy()
        last_obs = a.obs.cpu().numpy()
        assert torch.equal(mask, keep)                        # the caller's mask is read, never written
        for e, sl in zip(a.envs, _slices(a)):
            live = [g for g in range(sl.start, sl.stop) if g not in masked]
            d = sd[:, live]
            print(f'{e.env_id} fusion={fusion}: first dones at {sorted(int(np.argmax(d[:, j])) for j in range(len(live)) if d[:, j].any())}, '
                  f'{int((~d.any(axis=0)).sum())}/{len(live)} live envs never done')
            assert d[:-1].any(), f'{e.env_id}: no live env was done before the last step'
            assert not d.any(axis=0).all(), f'{e.env_id}: every live env was done'
            for g in range(sl.start, sl.stop):
                od, idim = e.obs_dim, e.info_dim
                # padding columns of caller buffers are left alone
                assert (ro[:, g, od:] == SENTINEL).all() and (ri[:, g, idim:] == SENTINEL).all()
                if g in masked:
                    assert (rr[:, g] == SENTINEL).all() and (rd[:, g] == 9).all()
                    assert (ro[:, g] == SENTINEL).all() and (ri[:, g] == SENTINEL).all()
                    assert np.array_equal(after[g], before[g]) and np.array_equal(last_obs[g], obs_before[g])
                    assert np.array_equal(after[g], ss[-1][g])
                    continue
                k = int(np.argmax(sd[:, g])) if sd[:, g].any() else T - 1     # the last step this env runs
                assert np.array_equal(rr[:k + 1, g], sr[:k + 1, g]) and np.array_equal(rd[:k + 1, g], sd[:k + 1, g])
                assert np.array_equal(ro[:k + 1, g, :od], so[:k + 1, g, :od])
                assert np.array_equal(ri[:k + 1, g, :idim], si[:k + 1, g, :idim])
                assert np.array_equal(after[g], ss[k][g])     # the state right after its first done step
                assert not rr[k + 1:, g].any() and (rd[k + 1:, g] == 1).all() and not ri[k + 1:, g, :idim].any()
                assert (ro[k + 1:, g, :od] == so[k, g, :od]).all()
                assert np.array_equal(last_obs[g, :od], so[k, g, :od])
        a.close(), b.close()
    finally:
        _fusion(1)


def test_group_action_repeat():
    """(N, A) actions with steps=4: the same action block four times"""
    a, b, acts = _pair(SEGS)
    o, r, d, i = a.rollout(acts[0], steps=4)
    assert o is a.obs and i is None and a.last_rollout_fused
    ro, rr, rd = _np(o, r, d)
    so, sr, sd, si = _stepped(b, acts[0].expand(4, -1, -1))
    assert np.array_equal(ro, so[-1]) and np.array_equal(rr, sr) and np.array_equal(rd, sd)
    _assert_same_envs(a, b)
    a.close(), b.close()


def test_mixed_state_calls_and_branching():
    import torch
    a, b, acts = _pair(SEGS, auto_reset=False)
    n = a.num_envs
    sl0, sl1 = _slices(a)
    # round trip: a moves on, its rows in a shuffled global order go into the twin
    for t in range(2):
        a.step(acts[t])
    ids = np.random.default_rng(3).permutation(n)
    rows = a.state_rows(env_ids=ids)
    assert tuple(rows.shape) == (n, a.state_dim) and rows.dtype == torch.float64
    assert a.state_dim == max(e.state_dim for e in a.envs)
    sm = a.state_mask.cpu().numpy()
    assert sm.shape == (n, a.state_dim) and sm.dtype == np.bool_
    for e, sl in zip(a.envs, _slices(a)):
        assert sm[sl, :e.state_dim].all() and not sm[sl, e.state_dim:].any()
    assert not rows.cpu().numpy()[~sm[ids]].any()                         # zero past each segment's own state_dim
    b.load_state(rows, ids)
    for ea, eb in zip(a.envs, b.envs):
        assert np.array_equal(ea.get_state(), eb.get_state())
    full = a.state_rows().cpu().numpy()
    assert np.array_equal(full[ids], rows.cpu().numpy())
    for e, sl in zip(a.envs, _slices(a)):
        assert np.array_equal(full[sl, :e.state_dim], e.get_state())
    # reset with global ids = the per-segment resets
    gids, grow = [33, 2, 21, 20, 7], [11, 4, 9, 0, 25]
    oa = a.reset(env_ids=gids, ref_index=grow)
    b.envs[0].reset([2, 20, 7], [4, 0, 25])
    b.envs[1].reset([12, 0], [11, 9])
    assert oa is a.obs and np.array_equal(a.obs.cpu().numpy()[gids], b.obs.cpu().numpy()[gids])   # the rows the reset wrote
    for ea, eb in zip(a.envs, b.envs):
        assert np.array_equal(ea.get_state(), eb.get_state())
    # branching: one env per segment cloned over three others of its segment,
    # then a rollout that gives each clone its source's action rows
    src, dst = [2, 2, 2, 23, 23, 23], [5, 17, 20, 21, 30, 33]
    a.clone_envs(src, dst)
    plan = acts[2:10].clone()
    plan[:, dst] = plan[:, src]
    o, r, d, _ = a.rollout(plan, obs='all')
    assert a.last_rollout_fused
    ro, rr, rd = _np(o, r, d)
    assert np.array_equal(rr[:, dst], rr[:, src]) and np.array_equal(rd[:, dst], rd[:, src])
    assert np.array_equal(ro[:, dst], ro[:, src])
    assert not np.array_equal(rr[:, 5], rr[:, 6])                          # other envs go their own way
    st = a.state_rows().cpu().numpy()
    assert np.array_equal(st[dst], st[src])
    with pytest.raises(ValueError):
        a.clone_envs([2], [25])                                            # a cross-segment pair
    with pytest.raises(ValueError):
        a.clone_envs(23, [5, 30])
    a.close(), b.close()


def test_mixed_rollout_refusals():
    import torch
    from bioimitation import _lib
    from bioimitation.vector_env import MixedVectorEnv
    m = MixedVectorEnv([(M2D, 3), (T2D, 2)], precision=64, seed=1, auto_reset=True)
    n, A = m.num_envs, m.action_dim
    z = lambda *s, dtype=m.dtype: torch.zeros(s, dtype=dtype, device=m.device)
    with pytest.raises(ValueError):
        m.rollout(z(4, n - 1, A))                                          # a wrong shape
    with pytest.raises(ValueError):
        m.rollout(z(4, n, A + 1))
    with pytest.raises(ValueError):
        m.rollout(z(n, A))                                                 # (N, A) needs steps
    with pytest.raises(ValueError):
        m.rollout(z(4, n, A), steps=3)                                     # a steps mismatch
    with pytest.raises(ValueError):
        m.rollout(z(4, n, A), out={'rewards': z(4, n)})                    # an unknown out key
    with pytest.raises(ValueError):
        m.rollout(z(4, n, A), out={'info': z(4, n, m.info_dim)})           # not asked for
    with pytest.raises(ValueError):
        m.rollout(z(4, n, A), out={'reward': z(4, n, dtype=torch.float32)})   # the wrong dtype
    with pytest.raises(ValueError):
        m.rollout(z(4, n, A), out={'done': z(4, n)})
    with pytest.raises(ValueError):
        m.rollout(z(4, n, A), stop_at_done=True)                           # auto-reset is on
    with pytest.raises(ValueError):
        m.set_active_mask(torch.ones(n - 1, dtype=torch.uint8, device=m.device))
    m.close()
    rk = MixedVectorEnv([(M2D, 3), (T2D, 2)], config={'integrator': 'rk-merson'}, precision=64, seed=1)
    rk.envs[1].set_rk_budget(4)
    with pytest.raises(_lib.BioimError, match='bioim_rollout_group: a budgeted RK handle'):
        rk.rollout(z(4, n, A))
    rk.close()
