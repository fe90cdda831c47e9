"""Batched static optimization (bioim_static_opt,
bioimitation.static_optimization, VectorEnv.static_optimization) against the
BVLS reference of tests/so_reference.py (validated by
tests/test_static_opt_reference.py).

Shapes: Walking2D with n = 1, 17 (a second workgroup with one state) and 200
(13 workgroups, a partial last one); Running3D, LockedKnee3D and Palsy3D with
n = 64 (two muscle rounds: 22 or 19 muscles on 16 lanes).  Inputs as
so_reference._reference; a reference is computed once per (ID, n, problem) and
shared.

Bounds: capacity 5e-9 relative to max(1, row max); act 5e-9 absolute (the
suite's fiber bound, test_gpu_muscle_analysis.FIBER_TOL[64]; the reference's
input sensitivity, about 1e-11 per 1e-12 of input error, puts the expected
error near 1e-10 and below); tau_muscle and residual 5e-9 relative to
max(1, row max |tau|).  Values are compared, never active sets.  Observed
maxima are printed (DESIGN.md 5.15 lists them).
"""
import functools

import numpy as np
import pytest

import so_reference as R
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason='needs GPU')]

W2D, R3D, K3D, P3D = ('MuscleWalkingImitation2D-v0', 'MuscleRunningImitation3D-v0', 'MuscleLockedKneeImitation3D-v0',
                      'MusclePalsyImitation3D-v0')
SHAPES = [(W2D, 1), (W2D, 17), (W2D, 200), (R3D, 64), (K3D, 64), (P3D, 64)]
CORNER_N = 4
CORNER_FROM = {W2D: 17, R3D: 64, K3D: 64, P3D: 64}     # the reference record whose first states the corners use
TOL = 5e-9
INF = float('inf')
KEYS = ('act', 'residual', 'tau_muscle', 'capacity', 'status', 'tau')


@pytest.fixture(scope='module')
def solvers():
    """one StaticOptimization per ID, shared by the module's tests"""
    from bioimitation.static_optimization import StaticOptimization
    made = {}

    def get(env_id):
        if env_id not in made:
            made[env_id] = StaticOptimization(env_id)
        return made[env_id]
    yield get
    for so in made.values():
        so.close()


@functools.lru_cache(maxsize=None)
def _solution(env_id, n, rows=None, reserve=1.0, scale=1.0, lo=0.0, hi=1.0, passive=False):
    """the reference's solution of one problem on a record's states (read-only, shared)"""
    r = R._reference(env_id, n)
    idx = list(range(n)) if rows is None else list(rows)
    tau = r.tau[idx] * scale
    out = R.solve(r, tau=tau, reserve=np.array(reserve) if isinstance(reserve, tuple) else reserve, lo=lo, hi=hi,
                  passive=passive, rows=idx)
    out['tau'] = tau
    for a in out.values():
        a.setflags(write=False)
    return out


def _np(t):
    return t.double().cpu().numpy() if t.dtype.is_floating_point else t.cpu().numpy()


def _rel(out, ref, scale_of=None):
    """max |out - ref| / max(1, row max |scale_of|), rows = states"""
    s = ref if scale_of is None else scale_of
    out, ref, s = out.reshape(len(ref), -1), ref.reshape(len(ref), -1), s.reshape(len(ref), -1)
    return (np.abs(out - ref) / np.maximum(1.0, np.abs(s).max(1, keepdims=True))).max()


def _check(tag, got, ref, lo, hi, cap_ref=None):
    """the parity and the conditions every solved problem must meet; returns the largest pass count"""
    act, tm, res, st, tau = (_np(got[k]) for k in ('act', 'tau_muscle', 'residual', 'status', 'tau'))
    assert (st >= 0).all(), (tag, st[st < 0], np.where(st < 0)[0])
    assert (act >= lo).all() and (act <= hi).all(), tag
    e = dict(act=np.abs(act - ref['act']).max(), tau_muscle=_rel(tm, ref['tau_muscle'], ref['tau']),
             residual=_rel(res, ref['residual'], ref['tau']))
    if cap_ref is not None:
        cap = _np(got['capacity'])
        e['Fa'], e['Fp'] = _rel(cap[:, :, 0], cap_ref[0]), _rel(cap[:, :, 1], cap_ref[1])
    print(tag, 'max err', {k: f'{v:.2e}' for k, v in e.items()}, 'passes max', int(st.max()), 'mean', f'{st.mean():.1f}',
          'reference BVLS iterations max', int(ref['nit'].max()))
    assert (tau == ref['tau']).all()
    bal = np.abs(res + tm - tau) / np.maximum(1.0, np.abs(tau))
    assert bal.max() <= 1e-12, (tag, bal.max())
    # the parity bounds last, all of them: a miss must not hide the figures and conditions after it
    missed = {k: v for k, v in e.items() if not v < TOL}
    assert not missed, (tag, missed)
    return int(st.max())


@pytest.mark.parametrize('env_id,n', SHAPES)
def test_matches_bvls_reference(env_id, n, solvers):
    """capacity against the helper's Fa and Fp; act, tau_muscle and residual
    against the BVLS reference at reserves 1 and 100; every state solved
    (status >= 0), the cap at least 4x the most passes seen, residual +
    tau_muscle == tau"""
    so = solvers(env_id)
    r = R._reference(env_id, n)
    most, missed = 0, []
    for reserve in (1.0, 100.0):
        ref = _solution(env_id, n, reserve=reserve)
        got = so.solve(r.q, r.u, tau=r.tau, reserve=reserve, want=KEYS)
        assert got['act'].shape == (n, r.pk.nmuscle) and got['capacity'].shape == (n, r.pk.nmuscle, 2)
        assert got['status'].shape == (n,) and str(got['status'].dtype) == 'torch.int32'
        assert all(v.device == so.device for v in got.values())
        most = max(most, int(got['status'].max()))
        # a muscle without any moment arm (LockedKnee3D's 14 and 18: every point below the locked knee) has
        # B = 0 exactly and stays at lo exactly, whatever residual its rows keep
        assert (got['act'][:, np.where(~r.live.any(1))[0]] == 0.0).all()
        try:
            _check(f'{env_id} n={n} reserve={reserve:g}', got, ref, 0.0, 1.0, (r.Fa, r.Fp))
        except AssertionError as err:      # the other reserve and the conditions below are still checked
            missed.append(err)
    cap = 8 * r.pk.nmuscle        # include/bioim.h: the cap is 8 nmuscle passes
    assert 4 * most <= cap, (most, cap)
    # act alone (the default), and the target from accelerations: the ID launch first
    only = so.solve(r.q, r.u, tau=r.tau)
    assert set(only) == {'act'} and (only['act'] == so.solve(r.q, r.u, tau=r.tau, want=KEYS)['act']).all()
    viaid = so.solve(r.q, r.u, qdd=r.qdd, want=('act', 'tau'))
    assert _rel(_np(viaid['tau']), r.tau) < 1e-9          # the id_kernel test's own bound
    again = so.solve(r.q, r.u, tau=viaid['tau'], want=('act',))
    assert (again['act'] == viaid['act']).all()
    assert not missed, missed


@pytest.mark.parametrize('env_id,n', SHAPES[2:])
def test_solver_is_exact_on_its_own_inputs(env_id, n, solvers):
    """The solver alone, without the geometry's rounding between it and the
    oracle: act against BVLS on the kernel's own capacity and on dL/dq as
    bioim_muscle_eval reports it (the same device functions on the same
    frames), with the kernel's exact zeros on rigidly moved paths
    (so_reference.live_mask).  Bound: the parity bound on act, 5e-9; observed <= 3.4e-13."""
    from bioimitation.muscle_analysis import MuscleAnalysis
    so = solvers(env_id)
    r = R._reference(env_id, n)
    got = so.solve(r.q, r.u, tau=r.tau, want=KEYS)
    ma = MuscleAnalysis(env_id, precision=64)
    dL = _np(ma.eval(r.q, r.u, want=('dldq',))['dldq'])
    ma.close()
    act, cap = _np(got['act']), _np(got['capacity'])
    lam = R.row_weights(1.0, r.pk.ndof)
    worst = 0.0
    for i in range(n):
        B, c = R.system(cap[i, :, 0], cap[i, :, 1], np.where(r.live, dL[i], 0.0), False)
        worst = max(worst, np.abs(act[i] - R.solve_state(B, c, r.tau[i], lam, 0.0, 1.0)[0]).max())
    print(env_id, n, 'act against BVLS on the kernel\'s own inputs: max err', f'{worst:.2e}')
    assert worst < TOL


@pytest.mark.parametrize('env_id', [W2D, R3D, K3D, P3D])
def test_corners(env_id, solvers):
    import torch
    so = solvers(env_id)
    nrec = CORNER_FROM[env_id]
    r = R._reference(env_id, nrec)
    rows = tuple(range(CORNER_N))
    q, u, tau = r.q[:CORNER_N], r.u[:CORNER_N], r.tau[:CORNER_N]
    nd = r.pk.ndof
    # tau = c exactly (c = 0 without the passive forces), and reserve = inf on every row: act exactly 0
    got = so.solve(q, u, tau=np.zeros_like(tau), want=KEYS)
    assert (got['act'] == 0.0).all() and (got['status'] == 0).all() and (got['tau_muscle'] == 0.0).all()
    got = so.solve(q, u, tau=tau, reserve=INF, passive=True, want=KEYS)
    assert (got['act'] == 0.0).all() and (got['status'] == 0).all()
    c = got['tau_muscle']                                  # B 0 + c: the kernel's own passive force
    fp_tau = -np.einsum('imd,im->id', r.dL[:CORNER_N], r.Fp[:CORNER_N])
    assert _rel(_np(c), fp_tau) < TOL
    got = so.solve(q, u, tau=c, passive=True, want=KEYS)
    assert (got['act'] == 0.0).all() and (got['status'] == 0).all() and (got['residual'] == 0.0).all()
    # a tau scaled x100: many muscles saturate
    ref = _solution(env_id, nrec, rows=rows, scale=100.0)
    got = so.solve(q, u, tau=100.0 * tau, want=KEYS)
    _check(f'{env_id} corner tau x100', got, ref, 0.0, 1.0)
    sat = int((ref['act'] >= 1.0 - 1e-15).sum())
    print(env_id, 'tau x100: activations at 1:', int((_np(got['act']) == 1.0).sum()), 'reference', sat, 'of', ref['act'].size)
    assert sat >= 2 * CORNER_N                             # the corner is what it says: many muscles saturate
    # other bounds; the passive forces; a per-dof reserve with inf on two spanned rows
    ref = _solution(env_id, nrec, rows=rows, lo=0.01, hi=0.9)
    _check(f'{env_id} corner lo=0.01 hi=0.9', so.solve(q, u, tau=tau, lo=0.01, hi=0.9, want=KEYS), ref, 0.01, 0.9)
    ref = _solution(env_id, nrec, rows=rows, passive=True)
    _check(f'{env_id} corner passive', so.solve(q, u, tau=tau, passive=True, want=KEYS), ref, 0.0, 1.0)
    from test_gpu_muscle_analysis import _pack_span
    spanned = np.where(_pack_span(r.pk).any(0))[0]
    assert 4 <= len(spanned) < nd                          # the floating base is not spanned
    reserve = np.linspace(0.5, 2.0, nd)
    reserve[spanned[[0, -1]]] = INF
    ref = _solution(env_id, nrec, rows=rows, reserve=tuple(reserve))
    got = so.solve(q, u, tau=tau, reserve=torch.as_tensor(reserve), want=KEYS)
    _check(f'{env_id} corner per-dof reserve', got, ref, 0.0, 1.0)


def test_zero_capacity_muscles_stay_at_the_lower_bound(solvers):
    """Palsy3D has muscles with Fa = 0 exactly: their activation is exactly
    lo, whatever the others do"""
    so = solvers(P3D)
    r = R._reference(P3D, 64)
    rows = tuple(int(i) for i in np.where((r.Fa == 0.0).any(1))[0][:CORNER_N])
    assert len(rows) == CORNER_N
    idx = list(rows)
    zero = r.Fa[idx] == 0.0
    for lo in (0.0, 0.01):
        ref = _solution(P3D, 64, rows=rows, lo=lo)
        got = so.solve(r.q[idx], r.u[idx], tau=r.tau[idx], lo=lo, want=KEYS)
        _check(f'{P3D} zero capacity lo={lo:g}', got, ref, lo, 1.0)
        act, cap = _np(got['act']), _np(got['capacity'])
        assert (cap[:, :, 0][zero] == 0.0).all()
        assert (act[zero] == lo).all()
        assert (act[~zero] != lo).any()


def test_states_are_independent_and_calls_repeat(solvers):
    """state i solved alone equals row i of the n = 200 call bit for bit (its
    own workgroup, lane group and neighbours differ); a repeated call is
    bit-identical"""
    import torch
    so = solvers(W2D)
    r = R._reference(W2D, 200)
    full = so.solve(r.q, r.u, tau=r.tau, want=KEYS)
    again = so.solve(r.q, r.u, tau=r.tau, want=KEYS)
    for k in KEYS:
        assert torch.equal(full[k], again[k]), k
    for i in (0, 3, 15, 16, 17, 63, 64, 130, 191, 192, 199):
        one = so.solve(r.q[i:i + 1], r.u[i:i + 1], tau=r.tau[i:i + 1], want=KEYS)
        for k in KEYS:
            assert torch.equal(one[k][0], full[k][i]), (i, k)
    so3 = solvers(R3D)
    r3 = R._reference(R3D, 64)
    full = so3.solve(r3.q, r3.u, tau=r3.tau, want=KEYS)
    for i in (0, 5, 17, 63):
        one = so3.solve(r3.q[i:i + 1], r3.u[i:i + 1], tau=r3.tau[i:i + 1], want=KEYS)
        for k in KEYS:
            assert torch.equal(one[k][0], full[k][i]), (i, k)


def test_env_static_optimization_reads_the_envs(solvers):
    """VectorEnv.static_optimization(qdd=zeros) at the envs' state: bit for
    bit StaticOptimization.solve on state_rows' q and u"""
    import torch
    from bioimitation.packdef import state_row_slices
    from bioimitation.vector_env import VectorEnv
    n = 8
    env = VectorEnv(W2D, n, precision=64)
    pk = env.pack
    env.reset(ref_index=[3, 11, 19, 27, 35, 43, 51, 59])
    rng = np.random.default_rng(5)
    for _ in range(3):
        env.step(torch.as_tensor(rng.uniform(0, 1, size=(n, env.action_dim)), device=env.device))
    zeros = torch.zeros((n, pk.ndof), dtype=torch.float64, device=env.device)
    got = env.static_optimization(qdd=zeros, want=KEYS)
    s = env.state_rows()
    sl, _ = state_row_slices(pk.ndof, pk.nmuscle, pk.nact, pk.horizon)
    want = solvers(W2D).solve(s[:, sl['q']], s[:, sl['u']], qdd=zeros, want=KEYS)
    for k in KEYS:
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    assert (got['status'] >= 0).all() and (got['act'] > 0).any()
    ids = [6, 1, 4]
    part = env.static_optimization(tau=got['tau'][ids], env_ids=ids, want=('act', 'residual'))
    assert set(part) == {'act', 'residual'}
    assert torch.equal(part['act'], got['act'][ids]) and torch.equal(part['residual'], got['residual'][ids])
    env.close()


def test_env_static_optimization_is_a_read():
    """Twin envs, one with static_optimization() calls between steps: the
    next three steps agree bit for bit, and the realize-cache flags do not
    move"""
    import torch
    from bioimitation.vector_env import VectorEnv
    n = 8
    a, b = (VectorEnv(W2D, n, precision=64, seed=7) for _ in range(2))
    rows = [2, 10, 18, 26, 34, 42, 50, 58]
    rng = np.random.default_rng(6)
    acts = torch.as_tensor(rng.uniform(0, 1, size=(5, n, a.action_dim)), device=a.device)
    for e in (a, b):
        e.reset(ref_index=rows)
        for t in range(2):
            e.step(acts[t])
    flags = a.debug_plane('cache_ok').copy()
    assert flags.any()                     # the steps left a live cache to lose
    zeros = torch.zeros((n, a.pack.ndof), dtype=torch.float64, device=a.device)
    a.static_optimization(qdd=zeros, want=KEYS)
    a.static_optimization(tau=zeros[:2], env_ids=[5, 0], passive=True, want=('act',))
    assert (a.debug_plane('cache_ok') == flags).all()
    assert (b.debug_plane('cache_ok') == flags).all()
    for t in (2, 3, 4):
        ra, rb = a.step(acts[t]), b.step(acts[t])
        for x, y, what in zip(ra, rb, ('obs', 'reward', 'done', 'info')):
            assert torch.equal(x, y), (t, what)
    assert (a.debug_plane('cache_ok') == b.debug_plane('cache_ok')).all()
    a.close()
    b.close()


def test_refusals():
    """ValueError for a torque ID and for a precision=32 env, from the Python
    layer; the library's own eighth refusal (fp64 handles only) on a real fp32
    handle with muscles"""
    import ctypes as C
    import torch
    from bioimitation.static_optimization import StaticOptimization
    from bioimitation.vector_env import VectorEnv
    tq = StaticOptimization('TorqueWalkingImitation2D-v0')
    z = np.zeros((2, tq.ndof))
    with pytest.raises(ValueError, match='no muscles'):
        tq.solve(z, tau=z)
    tq.close()
    env = VectorEnv('TorqueWalkingImitation2D-v0', 2)
    env.reset(ref_index=[1, 2])
    with pytest.raises(ValueError, match='no muscles'):
        env.static_optimization(tau=z)
    env.close()
    env = VectorEnv(W2D, 2, precision=32)
    env.reset(ref_index=[1, 2])
    z = np.zeros((2, env.pack.ndof))
    with pytest.raises(ValueError, match='fp64 envs only'):
        env.static_optimization(qdd=z)
    t = torch.zeros((2, 16), dtype=torch.float64, device=env.device)
    p = C.c_void_p(t.data_ptr())
    assert env._L.bioim_static_opt(env._h, 2, p, None, p, None, 0.0, 1.0, 0, p, None, None, None, None) == -1
    err = env._L.bioim_last_error()
    assert err.startswith(b'bioim_static_opt:') and b'fp64 handles only' in err, err
    env.close()
