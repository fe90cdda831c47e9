"""Fused multi-step rollouts: ``VectorEnv.rollout`` over
bioim_rollout — T env steps from an action sequence, one launch of the
rollout kernel on the default step configuration, T launches from C
otherwise.  Every comparison is bitwise against a twin env that is stepped
T times.

37 envs at 16 envs per workgroup are two full workgroups and a partial one
of 5.  T_ROLL is the smallest rollout length at which, with the seeds and
rows below, every case of the bit-identity test has a done before its last
step (so the in-loop auto-reset runs) and an env that is never done: the
first done falls in step 39 of the rollout for the planar muscle model (fp64
and fp32), 21 for the spatial running model and 51 for the planar torque
model (found by stepping the twin drive on the GPU), so T_ROLL - 1 > 51.  The
tests print their done counts."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason='needs a HIP GPU')]

N = 37
WARM = 3            # ordinary steps first: the rollout starts from a valid realize cache
T_ROLL = 53
T_MAX = 60          # actions are always drawn for T_MAX steps, so a prefix does not depend on T
M2D, T2D, R3D = 'MuscleWalkingImitation2D-v0', 'TorqueWalkingImitation2D-v0', 'MuscleRunningImitation3D-v0'
PLANES = ('cache', 'cache_ok', 'vnw', 'resets')


def _drive(env_id, n):
    """reference rows (one per env) and (T_MAX, n, A) actions: muscle models
    U[0, 0.4], torque models the PD targets of the next reference row +
    N(0, 0.05) (test_gpu_parity's through-termination drive)"""
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


def _pair(env_id, n, precision=64, auto_reset=True, config=None, warm=WARM):
    """two envs of the same seed at the same state, WARM steps in, and the
    remaining actions on the device, (T_MAX - WARM, n, A)"""
    import torch
    from bioimitation.vector_env import VectorEnv
    rows, acts = _drive(env_id, n)
    envs = [VectorEnv(env_id, n, config=config, precision=precision, seed=5, auto_reset=auto_reset) for _ in range(2)]
    dev = torch.as_tensor(acts, device=envs[0].device, dtype=envs[0].dtype).contiguous()
    for e in envs:
        e.reset(ref_index=rows)
        for t in range(warm):
            e.step(dev[t])
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


def _close(*envs):
    for e in envs:
        e.close()


@pytest.mark.parametrize('env_id,precision', [(M2D, 64), (T2D, 64), (R3D, 64), (M2D, 32)])
def test_rollout_is_bit_identical_to_stepping(env_id, precision):
    """Auto-reset on; the rollout is issued as two calls (T - 5 and 5 steps),
    so the second starts from the state, realize cache and reset counters the
    first left.  Outputs, the final state and the debug planes are equal bit
    for bit, and the in-loop auto-reset really ran."""
    import torch
    a, b, acts = _pair(env_id, N, precision)
    assert a.launch['envs_per_workgroup'] == 16
    T = T_ROLL
    first = a.rollout(acts[:T - 5], obs='all', info=True)
    assert a.last_rollout_fused
    second = a.rollout(acts[T - 5:T], obs='all', info=True)
    assert a.last_rollout_fused
    ro, rr, rd, ri = _np(*(torch.cat([x, y]) for x, y in zip(first, second)))
    so, sr, sd, si = _stepped(b, acts[:T])
    assert rd.shape == (T, N) and rd.dtype == np.uint8 and ro.shape == (T, N, a.obs_dim)
    ever = sd.any(axis=0)
    print(f'{env_id} fp{precision}: {int(sd.sum())} dones in {T} steps, first at step {int(np.argmax(sd.any(axis=1)))}, '
          f'{int(ever.sum())}/{N} envs were done, {int(sd[:-1].sum())} before the last step')
    assert np.array_equal(rr, sr)
    assert np.array_equal(rd, sd)
    assert np.array_equal(ro, so)
    assert np.array_equal(ri, si)
    assert np.array_equal(a.obs.cpu().numpy(), b.obs.cpu().numpy())     # obs='all' leaves the last rows in self.obs too
    assert np.array_equal(a.get_state(), b.get_state())
    for name in PLANES:
        assert np.array_equal(a.debug_plane(name), b.debug_plane(name)), name
    assert a.reset_count() == b.reset_count()
    # a condition, not a skip: without a done before the last step the in-loop auto-reset did not run
    assert sd[:-1].any(), 'no env was done before the last step: the in-loop auto-reset was not exercised'
    assert not ever.all(), 'every env was done: no env ran the whole rollout without a reset'
    _close(a, b)


def test_rollout_last_obs_composes_with_step():
    """obs='last' (the default) writes self.obs and returns it; a step() after
    the rollout continues like the twin's; final_obs keeps the last step's rows"""
    a, b, acts = _pair(M2D, N)
    a.enable_final_obs()
    b.enable_final_obs()
    T = T_ROLL
    o, r, d, i = a.rollout(acts[:T])
    assert o is a.obs and i is None and a.last_rollout_fused
    so, sr, sd, si = _stepped(b, acts[:T])
    ro, rr, rd = _np(o, r, d)
    assert np.array_equal(ro, so[-1]) and np.array_equal(rr, sr) and np.array_equal(rd, sd)
    assert np.array_equal(a.final_obs.cpu().numpy(), b.final_obs.cpu().numpy())
    na, nb = a.step(acts[T]), b.step(acts[T])
    for x, y in zip(_np(*na), _np(*nb)):
        assert np.array_equal(x, y)
    o2, r2, d2, i2 = a.rollout(acts[T + 1:T + 3], obs=None, info=True)
    assert o2 is None and i2.shape == (2, N, a.info_dim)
    _close(a, b)


def test_action_repeat_equals_expanded_actions():
    n = 5
    a, b, acts = _pair(M2D, n)
    one = acts[0]
    ra = a.rollout(one, steps=6, obs='all', info=True)
    assert a.last_rollout_fused
    rb = b.rollout(one.expand(6, n, a.action_dim).contiguous(), obs='all', info=True)
    for x, y in zip(_np(*ra), _np(*rb)):
        assert x.shape[0] == 6 and np.array_equal(x, y)
    assert np.array_equal(a.get_state(), b.get_state())
    so, sr, sd, si = _stepped(b, one.expand(2, n, a.action_dim))     # and both go on alike
    ro, rr, rd, ri = _np(*a.rollout(one, steps=2, obs='all', info=True))
    assert np.array_equal(ro, so) and np.array_equal(rr, sr) and np.array_equal(rd, sd) and np.array_equal(ri, si)
    _close(a, b)


def _check_stop_at_done(env_id, push):
    """Auto-reset off, N = 20, the caller's active mask with env 3 masked out.
    Against a twin that is stepped on (the reference steps through done)."""
    import torch
    n, T, OFF = 20, T_ROLL, 3
    a, b, acts = _pair(env_id, n, auto_reset=False)
    if push:        # a push table: the host-loop path
        x = np.arange(0.0, 4.0, 0.03) + 0.0013
        y = np.random.default_rng(9).choice([-50.0, 50.0], size=(n, len(x)))
        a.set_perturbation(x, y)
        b.set_perturbation(x, y)
    mask = torch.ones(n, dtype=torch.uint8, device=a.device)
    mask[OFF] = 0
    mask_b = mask.clone()
    a.set_active_mask(mask)
    b.set_active_mask(mask_b)
    start = a.get_state()
    SENT = -7.0
    out = {'obs': torch.full((T, n, a.obs_dim), SENT, dtype=a.dtype, device=a.device),
           'reward': torch.full((T, n), SENT, dtype=a.dtype, device=a.device),
           'done': torch.full((T, n), 9, dtype=torch.uint8, device=a.device),
           'info': torch.full((T, n, a.info_dim), SENT, dtype=a.dtype, device=a.device)}
    res = a.rollout(acts[:T], obs='all', info=True, stop_at_done=True, out=out)
    assert a.last_rollout_fused == (not push)
    assert all(res[k] is out[name] for k, name in enumerate(('obs', 'reward', 'done', 'info')))
    ro, rr, rd, ri = _np(*res)
    so, sr, sd, si, ss = _stepped(b, acts[:T], want_state=True)
    final = a.get_state()
    live = [e for e in range(n) if e != OFF]
    first = {e: (int(np.argmax(sd[:, e])) if sd[:, e].any() else None) for e in live}
    stopped = [e for e in live if first[e] is not None and first[e] < T - 1]
    print(f'{env_id}{" with a push table" if push else ""}: first done per env {first}')
    assert stopped, 'no env was done before the last step: nothing froze'
    for e in live:
        k = T - 1 if first[e] is None else first[e]
        assert np.array_equal(rr[:k + 1, e], sr[:k + 1, e]) and np.array_equal(rd[:k + 1, e], sd[:k + 1, e]), e
        assert np.array_equal(ro[:k + 1, e], so[:k + 1, e]) and np.array_equal(ri[:k + 1, e], si[:k + 1, e]), e
        assert (rr[k + 1:, e] == 0).all() and (rd[k + 1:, e] == 1).all() and (ri[k + 1:, e] == 0).all(), e
        assert (ro[k + 1:, e] == so[k, e]).all(), e
        assert np.array_equal(final[e], ss[k, e]), e          # the state right after its first done
        assert np.array_equal(a.obs[e].cpu().numpy(), so[k, e]), e
    # the masked-out env: untouched state, untouched rows; the caller's mask object unchanged
    assert np.array_equal(final[OFF], start[OFF])
    assert (rr[:, OFF] == SENT).all() and (rd[:, OFF] == 9).all() and (ro[:, OFF] == SENT).all() and (ri[:, OFF] == SENT).all()
    assert torch.equal(mask, mask_b) and a._active is mask
    # the mask is per call: a second rollout steps the frozen envs again
    rd2 = _np(a.rollout(acts[T:T + 2], stop_at_done=False)[2])[0]
    assert rd2.shape == (2, n)
    _close(a, b)


@pytest.mark.parametrize('env_id', [M2D, R3D])
def test_stop_at_done_freezes_an_env_after_its_first_done(env_id):
    """(The planar torque model's first done of this drive falls in the last
    of the T_ROLL steps, where nothing can freeze after it; the freezing code
    is the rollout kernel's own and does not depend on the topology.)"""
    _check_stop_at_done(env_id, push=False)


def test_stop_at_done_on_the_host_loop_path():
    """the same with a push table: T launches of the push kernel from C, and a
    small kernel between them that does what the rollout kernel's loop does"""
    _check_stop_at_done(M2D, push=True)


def test_stop_at_done_with_auto_reset_is_refused():
    a, b, acts = _pair(M2D, 4, warm=0)
    with pytest.raises(ValueError, match='stop_at_done'):
        a.rollout(acts[:2], stop_at_done=True)
    a.set_auto_reset(False)
    a.rollout(acts[:2], stop_at_done=True)
    _close(a, b)


@pytest.mark.parametrize('kind', ['push', 'rk-merson'])
def test_host_loop_path_equals_stepping(kind):
    """A push table or the RK-Merson integrator: the same call loops over the
    existing step kernels from C; bit-equal to stepping, not fused."""
    n, T = 8, 4
    cfg = {'integrator': 'rk-merson'} if kind == 'rk-merson' else None
    a, b, acts = _pair(M2D, n, config=cfg)
    if kind == 'push':
        x = np.arange(0.0, 4.0, 0.03) + 0.0013
        y = np.random.default_rng(9).choice([-50.0, 50.0], size=(n, len(x)))
        a.set_perturbation(x, y)
        b.set_perturbation(x, y)
    ro, rr, rd, ri = _np(*a.rollout(acts[:T], obs='all', info=True))
    assert not a.last_rollout_fused
    so, sr, sd, si = _stepped(b, acts[:T])
    assert np.array_equal(rr, sr) and np.array_equal(rd, sd) and np.array_equal(ro, so) and np.array_equal(ri, si)
    assert np.array_equal(a.obs.cpu().numpy(), b.obs.cpu().numpy())
    assert np.array_equal(a.get_state(), b.get_state())
    if kind == 'rk-merson':
        from bioimitation._lib import BioimError
        a.set_rk_budget(6)
        with pytest.raises(BioimError, match='budgeted'):
            a.rollout(acts[:T])
    _close(a, b)


def test_buffers_are_validated_without_a_launch():
    import torch
    n, T = 6, 4
    a, b, acts = _pair(M2D, n, warm=0)
    before = a.get_state()
    A, O = a.action_dim, a.obs_dim
    good = lambda: torch.empty((T, n), dtype=a.dtype, device=a.device)
    bad = {
        'wrong dtype': {'reward': torch.empty((T, n), dtype=torch.float32, device=a.device)},
        'T - 1 rows': {'reward': torch.empty((T - 1, n), dtype=a.dtype, device=a.device)},
        'host tensor': {'reward': torch.empty((T, n), dtype=a.dtype)},
        'non-contiguous': {'reward': torch.empty((n, T), dtype=a.dtype, device=a.device).t()},
        'done dtype': {'done': torch.empty((T, n), dtype=torch.bool, device=a.device)},
        'obs rows': {'obs': torch.empty((T, n, O + 1), dtype=a.dtype, device=a.device)},
        'unknown name': {'rewards': good()},
    }
    for what, out in bad.items():
        with pytest.raises(ValueError):
            a.rollout(acts[:T], obs='all', out=out)
    with pytest.raises(ValueError):
        a.rollout(acts[:T], out={'info': torch.empty((T, n, a.info_dim), dtype=a.dtype, device=a.device)})   # info not asked for
    with pytest.raises(ValueError):
        a.rollout(torch.zeros((T, n - 1, A), dtype=a.dtype, device=a.device))
    with pytest.raises(ValueError):
        a.rollout(acts[0])                       # (N, A) without steps
    with pytest.raises(ValueError):
        a.rollout(acts[:T], steps=T + 1)
    with pytest.raises(ValueError):
        a.rollout(acts[:T], obs='first')
    assert np.array_equal(a.get_state(), before)     # nothing ran
    r = good()
    assert a.rollout(acts[:T], out={'reward': r})[1] is r
    _close(a, b)


def test_rollout_after_clone_gives_identical_columns():
    import torch
    n, T = 8, 5
    a, b, acts = _pair(M2D, n, auto_reset=False)
    a.clone_envs(0, range(1, n))
    plan = acts[:T, :1].expand(T, n, a.action_dim).contiguous()
    ro, rr, rd, ri = _np(*a.rollout(plan, obs='all', info=True))
    assert a.last_rollout_fused
    for e in range(1, n):
        assert np.array_equal(rr[:, e], rr[:, 0]) and np.array_equal(ro[:, e], ro[:, 0]), e
        assert np.array_equal(rd[:, e], rd[:, 0]) and np.array_equal(ri[:, e], ri[:, 0]), e
    # and the column is the stepped twin's env 0 under the same plan
    so, sr, sd, si = _stepped(b, plan)
    assert np.array_equal(rr[:, 0], sr[:, 0]) and np.array_equal(ro[:, 0], so[:, 0])
    _close(a, b)
