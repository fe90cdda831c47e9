"""The flat state row against the planes of the per-env record.

``VectorEnv.debug_plane`` copies one whole plane of the device state and
shares nothing with the kernels that gather and load flat rows, so it is the
second opinion on the row's layout: ``packdef.state_row_slices`` names where
each field sits in a row, and every row call (get_state, set_state,
state_rows, load_state) must agree with the planes under those slices.

Every comparison is exact.  3 envs on distinct reference rows, two steps of
random actions."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason='needs a HIP GPU')]

N = 3
M2D, T2D = 'MuscleWalkingImitation2D-v0', 'TorqueWalkingImitation2D-v0'
INT_FIELDS = ('istep', 'has_last', 'done')
# the planes the flat row does not hold (the realize-cache rows aside)
OTHER_PLANES = ('resets', 'pend', 'rkt', 'rkh', 'rka', 'cur', 'vnw', 'rkev', 'cache_ok')


def _make(env_id, precision, config):
    import torch
    from bioimitation.vector_env import VectorEnv
    env = VectorEnv(env_id, N, config=config, precision=precision, auto_reset=False)
    pk = env.pack
    rows = np.array([3, 40, 77], dtype=np.int32)
    env.reset(ref_index=rows)
    rng = np.random.default_rng(5)
    for t in range(2):
        if pk.nmuscle:
            a = rng.uniform(0.0, 0.3, size=(N, pk.nact))
        else:   # PD targets: the next reference row's coordinates, perturbed
            a = np.array([[pk.ref_q[int(r) + t + 1][pk.pd_coord[k]] for k in range(pk.nact)] for r in rows]) + \
                rng.normal(0.0, 0.02, size=(N, pk.nact))
        env.step(torch.as_tensor(a, device=env.device, dtype=env.dtype))
    return env


def _slices(env):
    from bioimitation.packdef import state_row_slices, STATE_ROW_FIELDS
    pk = env.pack
    sl, dim = state_row_slices(pk.ndof, pk.nmuscle, pk.nact, pk.horizon)
    assert dim == env.state_dim and tuple(sl) == STATE_ROW_FIELDS
    return sl


def _planes(env):
    """every plane of the record but the cache rows, by name"""
    from bioimitation.packdef import STATE_ROW_FIELDS
    return {name: env.debug_plane(name) for name in STATE_ROW_FIELDS + OTHER_PLANES}


def _synthetic(env, sl, base):
    """rows of distinct values, exact in fp32: base + 1000 e + k, the
    non-integer fields 1/4 above that"""
    S = base + 1000.0 * np.arange(N)[:, None] + np.arange(env.state_dim)[None, :]
    for f, s in sl.items():
        if f not in INT_FIELDS:
            S[:, s] += 0.25
    return S


def _check_row_fields(planes, sl, S, envs):
    """the planes hold rows S (one per env of ``envs``) in their own element types"""
    for f, s in sl.items():
        p = planes[f]
        count = s.stop - s.start
        for r, e in enumerate(envs):
            assert np.array_equal(p[:count, e], S[r, s].astype(p.dtype)), (f, e)


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('env_id,precision,config', [
    (M2D, 64, None), (M2D, 32, None), (T2D, 64, None), (M2D, 64, {'integrator': 'rk-merson'})],
    ids=['muscle-fp64', 'muscle-fp32', 'torque-fp64', 'muscle-rk'])
def test_flat_row_matches_planes(env_id, precision, config):
    import torch
    from bioimitation._lib import BioimError
    env = _make(env_id, precision, config)
    pk, sl = env.pack, _slices(env)
    real = np.float32 if precision == 32 else np.float64

    # 1. row equals planes
    planes = _planes(env)
    g = env.get_state()
    for f, s in sl.items():
        p = planes[f]
        count = s.stop - s.start
        assert p.dtype == (np.int32 if f in INT_FIELDS else np.float64 if f in ('t', 'hrk') else real), f
        assert p.shape[0] >= max(count, 1), f
        for e in range(N):
            assert np.array_equal(g[e, s], p[:count, e].astype(np.float64)), (f, e)
    if pk.nmuscle == 0:
        assert sl['act'].stop == sl['act'].start and planes['act'].shape == (1, N)
    if config:
        assert (planes['hrk'] != 0).all(), 'the RK step size is not carried: the hrk field shows nothing'
    assert np.array_equal(env.state_rows().cpu().numpy(), g)
    assert np.array_equal(env.state_rows(env_ids=[2, 0, 2]).cpu().numpy(), g[[2, 0, 2]])

    # 2. set_state writes the right planes, and nothing but them and the two flags
    ones = np.ones((1, N), dtype=np.int32)
    env.debug_plane('pend', ones)
    env.debug_plane('cache_ok', ones)
    S = _synthetic(env, sl, 0.0)
    env.set_state(S)
    after = _planes(env)
    _check_row_fields(after, sl, S, range(N))
    assert not after['pend'].any() and not after['cache_ok'].any()
    for name in ('vnw', 'resets', 'rkev', 'rkt', 'rkh', 'rka', 'cur'):
        assert _bits_equal(after[name], planes[name]), name
    for f, s in sl.items():     # the rows of a plane past the field's count
        count = s.stop - s.start
        assert _bits_equal(after[f][count:], planes[f][count:]), f
    assert np.array_equal(env.get_state(), S)

    # 3. load_state touches only the listed env
    env.debug_plane('cache_ok', ones)
    before = _planes(env)
    S2 = _synthetic(env, sl, 5000.0)[:1]
    env.load_state(torch.from_numpy(S2).to(env.device), [2])
    after = _planes(env)
    _check_row_fields(after, sl, S2, [2])
    assert after['cache_ok'].tolist() == [[1, 1, 0]]
    for name, p in before.items():
        assert _bits_equal(after[name][:, :2], p[:, :2]), name
        if name not in sl and name != 'cache_ok':
            assert _bits_equal(after[name], p), name

    # 4. get_state refuses while an env is suspended mid-step; state_rows does not
    env.debug_plane('pend', np.array([[0, 1, 0]], dtype=np.int32))
    with pytest.raises(BioimError, match='suspended mid-step'):
        env.get_state()
    S[2] = S2[0]
    assert np.array_equal(env.state_rows().cpu().numpy(), S)
    env.debug_plane('pend', np.zeros((1, N), dtype=np.int32))

    # 5. set_rk_counters writes the rkev plane alone
    before = _planes(env)
    env.set_rk_counters(7, 9)
    after = _planes(env)
    assert (after['rkev'] == np.uint64((9 << 32) | 7)).all() and after['rkev'].shape == (1, N)
    for name, p in before.items():
        if name != 'rkev':
            assert _bits_equal(after[name], p), name
    assert env.eval_count() == 7 * N and env.finished_count() == 9 * N
    env.close()
