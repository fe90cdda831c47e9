"""Batched computed muscle control (bioim_cmc,
bioimitation.computed_muscle_control, VectorEnv.computed_muscle_control,
CMCDrive) against the reference of tests/cmc_reference.py (validated by
tests/test_cmc_reference.py).

Models: Walking2D (14 muscles, one per lane), Running3D (22 muscles, two per
lane), Palsy3D (the file's own curves).  n = 1, 17 and 33: a lone state, a
partial last workgroup, more than two workgroups at 16 states each.  The
reference is computed once per model (33 states) and shared.

Bounds.
  Against the reference: force_range and force as F / F0, tau_muscle and
  residual per max(1, |row|), within the suite's 5e-9, or 100 x what one ulp
  on q moves the reference's own values by where that exceeds 5e-11
  (cmc_reference.bound; the envelopes are about 1e-13, so 5e-9 holds:
  DESIGN.md 5.22 lists them with the observed errors).
  Root property, whatever path the iteration took: with the reference's
  predictor |P_ref(e_gpu) - F*_gpu| <= (ftol + that bound) F0 on every pair.
  Cross-kernel: bioim_muscle_eval at (q1, state_end) returns `predicted` as
  its tendon force within 4 ulp (the same device function on the same
  numbers, inlined into two kernels).
  Identities (a state alone, a repeated call, q1 given or not, outputs not
  asked for, the own-state call, a read of the envs): bit for bit.
Observed values are printed."""
import numpy as np
import pytest

import cmc_reference as R
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason='needs GPU')]

W2D, R3D, P3D = 'MuscleWalkingImitation2D-v0', 'MuscleRunningImitation3D-v0', 'MusclePalsyImitation3D-v0'
MODELS = [W2D, R3D, P3D]
KEYS = ('excitation', 'force', 'force_range', 'predicted', 'state_end', 'tau_muscle', 'residual', 'status',
        'root_status', 'tau')
COMPARED = ('force_range', 'force', 'tau_muscle', 'residual')


@pytest.fixture(scope='module')
def solvers():
    """one ComputedMuscleControl per ID, shared by the module's tests"""
    from bioimitation.computed_muscle_control import ComputedMuscleControl
    made = {}

    def get(env_id):
        if env_id not in made:
            made[env_id] = ComputedMuscleControl(env_id)
        return made[env_id]
    yield get
    for s in made.values():
        s.close()


def _np(t):
    return t.double().cpu().numpy() if t.dtype.is_floating_point else t.cpu().numpy()


def _solve(cmc, r, rows, **kw):
    return cmc.solve(r.q[rows], r.u[rows], r.act[rows], r.lce[rows], tau=r.tau[rows], want=KEYS, **kw)


_full = {}


def _case(env_id, solvers):
    """the n = 33 result on the reference's states (computed once per model, shared)"""
    if env_id not in _full:
        r = R._reference(env_id)
        _full[env_id] = _solve(solvers(env_id), r, slice(0, R.NS))
    return _full[env_id]


def _brackets(r):
    b = np.array([r.mus.bracket(m) for m in range(r.pk.nmuscle)])
    return b[:, 0], b[:, 1]


def _check_roots(tag, r, got, act, lce, L0, L1, bound):
    """the root property and the conditions on e and root_status for the states of `got` (numpy)"""
    e, F, fr, rs = got['excitation'], got['force'], got['force_range'], got['root_status']
    el, eh = _brackets(r)
    assert (rs >= 0).all(), (tag, np.argwhere(rs < 0))
    assert np.isfinite(e).all() and (e >= el).all() and (e <= eh).all(), tag
    at_min, at_max = F == fr.min(2), F == fr.max(2)
    up = fr[..., 0] <= fr[..., 1]
    assert ((rs == 0) == (at_min | at_max)).all(), tag
    end = np.where(at_min == up, el, eh)      # the minimum's end is the lower one where the range goes up
    assert (e[at_min | at_max] == end[at_min | at_max]).all(), tag
    worst = 0.0
    for i in range(len(e)):
        for m in range(r.pk.nmuscle):
            P = r.mus.predict(m, act[i, m], lce[i, m], L0[i, m], L1[i, m], e[i, m])[0]
            worst = max(worst, abs(P - F[i, m]) / r.f0[m])
    print(f'{tag}: root property, worst |P_ref(e) - F*| / F0 = {worst:.2e} (allowed {R.FTOL + bound:.2e}); evaluations '
          f'max {rs.max()}, mean over the solved {rs[rs > 0].mean() if (rs > 0).any() else 0:.1f}; on a bound '
          f'{100 * (rs == 0).mean():.0f} %')
    assert worst <= R.FTOL + bound, (tag, worst)


@pytest.mark.parametrize('n', [1, 17, 33])
@pytest.mark.parametrize('env_id', MODELS)
def test_matches_the_reference(env_id, n, solvers):
    r = R._reference(env_id)
    got = _case(env_id, solvers) if n == R.NS else _solve(solvers(env_id), r, slice(0, n))
    nm, nd = r.pk.nmuscle, r.pk.ndof
    shapes = dict(excitation=(n, nm), force=(n, nm), force_range=(n, nm, 2), predicted=(n, nm), state_end=(n, nm, 2),
                  tau_muscle=(n, nd), residual=(n, nd), status=(n,), root_status=(n, nm), tau=(n, nd))
    for k in KEYS:
        assert tuple(got[k].shape) == shapes[k], k
    assert str(got['status'].dtype) == 'torch.int32' and str(got['root_status'].dtype) == 'torch.int32'
    g = {k: _np(got[k]) for k in KEYS}
    assert (g['status'] >= 0).all(), g['status']
    assert (g['tau'] == r.tau[:n]).all()
    bound = R.bound(env_id)
    err = R.scaled_errors(r, g, {k: r.out[k][:n] for k in COMPARED})
    print(f'{env_id} n={n}: worst errors ' + ', '.join(f'{k} {v:.2e}' for k, v in err.items()) +
          f'; bound {bound:.1e}; envelope ' + ', '.join(f'{k} {v:.1e}' for k, v in R.envelope(env_id).items()) +
          f'; solver passes max {g["status"].max()}')
    bal = np.abs(g['residual'] + g['tau_muscle'] - g['tau']) / np.maximum(1.0, np.abs(g['tau']))
    assert bal.max() <= 1e-12
    missed = {k: v for k, v in err.items() if not v <= bound}
    assert not missed, (env_id, n, missed)


@pytest.mark.parametrize('env_id', MODELS)
def test_root_property(env_id, solvers):
    r = R._reference(env_id)
    g = {k: _np(v) for k, v in _case(env_id, solvers).items()}
    _check_roots(f'{env_id} n={R.NS}', r, g, r.act, r.lce, r.out['L0'], r.out['L1'], R.bound(env_id))
    assert (g['root_status'] > 0).sum() >= g['root_status'].size // 10      # the comparison is not one of fixed muscles


@pytest.mark.parametrize('env_id', MODELS)
def test_state_end_reproduces_predicted_in_muscle_eval(env_id, solvers):
    import torch
    from bioimitation.muscle_analysis import MuscleAnalysis
    r = R._reference(env_id)
    got = _case(env_id, solvers)
    ma = MuscleAnalysis(env_id)
    q, u = (torch.tensor(x, device=ma.device) for x in (r.q, r.u))
    fib = ma.eval(q + R.WINDOW * u, u, got['state_end'][:, :, 0].contiguous(), got['state_end'][:, :, 1].contiguous(),
                  want=('fiber',))['fiber']
    ft, pred = _np(fib[:, :, 2]), _np(got['predicted'])
    ulps = np.abs(ft - pred) / np.spacing(np.abs(pred))
    print(f'{env_id}: muscle_eval at state_end vs predicted, worst {ulps.max():.1f} ulp')
    ma.close()
    assert (ulps <= 4).all()


def test_invariances(solvers):
    import torch
    for env_id, singles in ((W2D, (0, 5, 15, 16, 17, 32)), (R3D, (0, 16, 31, 32)), (P3D, (3, 32))):
        cmc, r = solvers(env_id), R._reference(env_id)
        full = _case(env_id, solvers)
        again = _solve(cmc, r, slice(0, R.NS))
        for k in KEYS:
            assert torch.equal(full[k], again[k]), (env_id, k)
        for i in singles:
            one = _solve(cmc, r, slice(i, i + 1))
            for k in KEYS:
                assert torch.equal(one[k][0], full[k][i]), (env_id, i, k)
        q, u = (torch.tensor(x, device=cmc.device) for x in (r.q, r.u))
        given = _solve(cmc, r, slice(0, R.NS), q1=q + R.WINDOW * u)
        for k in KEYS:
            assert torch.equal(given[k], full[k]), (env_id, 'q1', k)
        part = cmc.solve(r.q, r.u, r.act, r.lce, tau=r.tau, want=('root_status', 'excitation', 'residual'))
        assert set(part) == {'root_status', 'excitation', 'residual'}
        for k in part:
            assert torch.equal(part[k], full[k]), (env_id, 'part', k)
        only = cmc.solve(r.q, r.u, r.act, r.lce, tau=r.tau)
        assert set(only) == {'excitation'} and torch.equal(only['excitation'], full['excitation'])
        # another window and substep count is another problem (the arguments arrive)
        other = _solve(cmc, r, slice(0, 4), window=0.02, nsub=5)
        assert not torch.equal(other['force_range'], full['force_range'][:4])
        empty = cmc.solve(r.q[:0], r.u[:0], r.act[:0], r.lce[:0], tau=r.tau[:0], want=KEYS)
        assert empty['excitation'].shape == (0, r.pk.nmuscle) and empty['root_status'].shape == (0, r.pk.nmuscle)


def _stepped_env(env_id, n, rows, seed, steps=3):
    import torch
    from bioimitation.vector_env import VectorEnv
    env = VectorEnv(env_id, n, precision=64, seed=7)
    env.reset(ref_index=rows)
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        env.step(torch.as_tensor(rng.uniform(0, 1, size=(n, env.action_dim)), device=env.device))
    return env


@pytest.mark.parametrize('env_id,n', [(W2D, 8), (R3D, 4)])
def test_env_call_reads_the_envs(env_id, n, solvers):
    """VectorEnv.computed_muscle_control at the envs' state: bit for bit
    ComputedMuscleControl.solve on the state rows; a twin env that is not
    asked steps on bit for bit, with the same cache_ok plane."""
    import torch
    from bioimitation.packdef import state_row_slices
    rows = [3 + 8 * i for i in range(n)]
    a, b = (_stepped_env(env_id, n, rows, seed=5, steps=2) for _ in range(2))
    pk = a.pack
    flags = a.debug_plane('cache_ok').copy()
    rng = np.random.default_rng(8)
    qdd = torch.as_tensor(rng.normal(0, 2, size=(n, pk.ndof)), device=a.device)
    got = a.computed_muscle_control(qdd=qdd, want=KEYS)
    s = a.state_rows()
    sl, _ = state_row_slices(pk.ndof, pk.nmuscle, pk.nact, pk.horizon)
    want = solvers(env_id).solve(s[:, sl['q']], s[:, sl['u']], s[:, sl['act']], s[:, sl['lce']], qdd=qdd, want=KEYS)
    for k in KEYS:
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    assert (got['status'] >= 0).all() and (got['root_status'] >= 0).all() and (got['root_status'] > 0).any()
    ids = [n - 2, 1, 2]
    part = a.computed_muscle_control(tau=got['tau'][ids], env_ids=ids, want=('excitation', 'force'))
    assert torch.equal(part['excitation'], got['excitation'][ids]) and torch.equal(part['force'], got['force'][ids])
    assert (a.debug_plane('cache_ok') == flags).all() and (b.debug_plane('cache_ok') == flags).all()
    acts = torch.as_tensor(rng.uniform(0, 1, size=(3, n, a.action_dim)), device=a.device)
    for t in range(3):
        ra, rb = a.step(acts[t]), b.step(acts[t])
        for x, y, what in zip(ra, rb, ('obs', 'reward', 'done', 'info')):
            assert torch.equal(x, y), (t, what)
    assert (a.debug_plane('cache_ok') == b.debug_plane('cache_ok')).all()
    a.close()
    b.close()


@pytest.mark.parametrize('env_id,n', [(W2D, 8), (R3D, 4)])
def test_drive_closes_the_loop(env_id, n):
    """10 steps of venv.step(CMCDrive(venv)()).  Per step, at the gathered
    state rows (a stateless check: no trajectory enters it): the drive's
    action is the own-state call's excitation at q''*, finite and in [0, 1];
    its forces and ranges meet the reference's within the bound and the root
    property holds."""
    import torch
    from bioimitation import CMCDrive
    from bioimitation.packdef import state_row_slices
    env = _stepped_env(env_id, n, [5 + 9 * i for i in range(n)], seed=11, steps=1)
    pk = env.pack
    drive = CMCDrive(env)
    r = R.model(env_id)
    bound = R.bound(env_id)
    sl, _ = state_row_slices(pk.ndof, pk.nmuscle, pk.nact, pk.horizon)
    worst = dict.fromkeys(COMPARED, 0.0)
    for t in range(10):
        rows = env.state_rows()
        action = drive()
        assert action.shape == (n, pk.nmuscle) and action.dtype == env.dtype and action.device == env.device
        full = env.computed_muscle_control(qdd=drive.target(rows), rows=rows, want=KEYS)
        assert torch.equal(full['excitation'], action)
        g = {k: _np(v) for k, v in full.items()}
        assert np.isfinite(g['excitation']).all() and (g['excitation'] >= 0).all() and (g['excitation'] <= 1).all()
        assert (g['status'] >= 0).all()
        s = _np(rows)
        q, u, act, lce = (s[:, sl[f]] for f in ('q', 'u', 'act', 'lce'))
        ref = [R.solve_state(r, q[i], u[i], act[i], lce[i], g['tau'][i], roots=False) for i in range(n)]
        ref = {k: np.stack([x[k] for x in ref]) for k in ref[0]}
        err = R.scaled_errors(r, g, ref)
        worst = {k: max(worst[k], err[k]) for k in COMPARED}
        assert all(v <= bound for v in err.values()), (env_id, t, err)
        _check_roots(f'{env_id} drive step {t}', r, g, act, lce, ref['L0'], ref['L1'], bound)
        env.step(action)
    print(f'{env_id}: 10 closed-loop steps, worst errors against the reference ' +
          ', '.join(f'{k} {v:.2e}' for k, v in worst.items()))
    env.close()


def test_refusals():
    """ValueError for a torque ID and for a precision=32 env, from the Python
    layer; the library's own last refusal (fp64 handles only) on a real fp32
    handle with muscles"""
    import ctypes as C
    import torch
    from bioimitation import CMCDrive
    from bioimitation.vector_env import VectorEnv
    env = VectorEnv('TorqueWalkingImitation2D-v0', 2)
    env.reset(ref_index=[1, 2])
    z = np.zeros((2, env.pack.ndof))
    with pytest.raises(ValueError, match='no muscles'):
        env.computed_muscle_control(tau=z)
    with pytest.raises(ValueError, match='no muscles'):
        CMCDrive(env)
    env.close()
    env = VectorEnv(W2D, 2, precision=32)
    env.reset(ref_index=[1, 2])
    z = np.zeros((2, env.pack.ndof))
    with pytest.raises(ValueError, match='fp64 envs only'):
        env.computed_muscle_control(qdd=z)
    t = torch.zeros((2, 32), dtype=torch.float64, device=env.device)
    p = C.c_void_p(t.data_ptr())
    assert env._L.bioim_cmc(env._h, 2, p, p, p, p, None, p, None, 0.01, 20, 0.0, 1.0, 1e-6, 30, p, None, None, None,
                            None, None, None, None, None) == -1
    err = env._L.bioim_last_error()
    assert err.startswith(b'bioim_cmc:') and b'fp64 handles only' in err, err
    env.close()
