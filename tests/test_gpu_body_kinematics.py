"""Batched body kinematics (bioim_body_kin, bioimitation.body_kinematics,
VectorEnv.body_kinematics) on the GPU.

States: tests/bk_reference.py::Yardstick.draw_states, 33 per model: the oracle
reset at reference rows and stepped 3 times with random actions, so u and q''
are far from 0 (asserted).  Models: Walking2D (planar), TorqueLockedKnee2D
(no muscles, merged leg), Running3D, LockedKnee3D (merged leg), Palsy3D.
n = 1, 17 and 33: a lone state, a second workgroup holding one state, a third.

Bounds.
  Against the yardstick (the oracle's own report of the realized state, the
  rest formed in numpy from it; tests/bk_reference.py), with the oracle's own
  q'': every output within 5e-9 x max(1, the row's largest magnitude), a row
  being one state's block of one output.  Observed: DESIGN.md 5.20.
  Identities: bit for bit where the kernel runs one piece of code on the same
  numbers (a point at a body's origin / mass centre against that body's origin
  / com row; u or qdd None against zeros; a state alone against its row of a
  larger call; a repeated call).  momentum[0] against m x system velocity:
  8 eps x max(1, |row|): the kernel divides the same sum by m (one rounding)
  and the test multiplies it back (a second), with m summed in another order
  (a few more).  Kinetic energy against u . (M u) / 2 from bioim_id_eval:
  1e-12 x max(1, KE): two fp64 sums of some hundred products each with no
  cancellation beyond their own size (eps x 100 terms, x 40 to spare).
  rot orthonormal to 1e-14 (nine products and sums of entries <= 1); the
  orient angles rebuild rot to 1e-13 (atan2, sin and cos at a few ulp each,
  through three products, away from the gimbal lock a gait never reaches).
  Chain rule, Running3D: central differences at h = 1e-6 within 1e-6 x max(1,
  |row|): h^2 truncation and 1e-16 / h rounding are both well below it.
  fp32 handle against fp64, Walking2D, n = 17: 4 x the observed worst error
  relative to max(1, |row|) (FP32_OBSERVED; fp32 rounding varies with the
  state set).
Observed values are printed."""
import functools

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason='needs GPU')]

W2D, TLK2D, R3D, LK3D, P3D = ('MuscleWalkingImitation2D-v0', 'TorqueLockedKneeImitation2D-v0',
                              'MuscleRunningImitation3D-v0', 'MuscleLockedKneeImitation3D-v0',
                              'MusclePalsyImitation3D-v0')
MODELS = [W2D, TLK2D, R3D, LK3D, P3D]
NS = 33
KEYS = ('origin', 'com', 'orient', 'rot', 'system', 'momentum', 'energy', 'point')
BOUND = 5e-9
EPS = np.finfo(np.float64).eps
FP32_OBSERVED = 4.41e-7    # worst |fp32 - fp64| / max(1, |row|) over all outputs, Walking2D, n = 17


def _np(t):
    return t.double().cpu().numpy()


def _rowmax(a):
    """max(1, largest magnitude) per state (a: [n, ...])"""
    return np.maximum(1.0, np.abs(a.reshape(a.shape[0], -1)).max(axis=1)) if a.size else np.ones(a.shape[0])


def _points(ys):
    """19 points (past the 16 lanes): a ground point, two on one body, a
    body's origin (6), a body's own mass centre (7), then one per body round
    the model with offsets of a foot's size."""
    rng = np.random.default_rng(7)
    b = ys.bodies
    pts = [('calcn_r', (0.18, 0.0, 0.0)), ('ground', (0.3, -0.2, 0.7)), ('calcn_r', (0.05, 0.02, -0.03)),
           ('torso', (0.0, 0.4, 0.0)), ('pelvis', (-0.1, 0.05, 0.08)), ('toes_l', (0.03, 0.0, 0.01)),
           ('tibia_l', (0.0, 0.0, 0.0)), ('femur_r', tuple(ys.os_com[b.index('femur_r')]))]
    while len(pts) < 19:
        pts.append((b[len(pts) % len(b)], tuple(rng.uniform(-0.2, 0.2, size=3))))
    return pts


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(env_id):
    """The model's analysis object, test states, yardstick values and the
    n = 33 result (computed once, shared, read-only)."""
    import oracle
    import bk_reference as B
    from bioimitation.body_kinematics import BodyKinematics
    c = Case()
    c.ys = B.yardstick(oracle, env_id)
    c.bk = BodyKinematics(env_id)
    c.q, c.u, c.a, reps = c.ys.draw_states(NS, seed=31)
    c.pts = _points(c.ys)
    ref = [c.ys.eval(c.q[i], reps[i], c.pts) for i in range(NS)]
    c.ref = {k: np.stack([r[k] for r in ref]) for k in KEYS}
    refl = [c.ys.eval(c.q[i], reps[i], c.pts, local=True) for i in range(NS)]
    c.ref_local = {k: np.stack([r[k] for r in refl]) for k in KEYS}
    c.out_t = c.bk.eval(c.q, c.u, c.a, points=c.pts, want=KEYS)
    c.out = {k: _np(v) for k, v in c.out_t.items()}
    for a in list(vars(c).values()) + list(c.ref.values()) + list(c.ref_local.values()) + list(c.out.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def _compare(env_id, got, ref, n, tag):
    worst = {}
    for k in KEYS:
        g, r = got[k].reshape(n, -1), ref[k][:n].reshape(n, -1)
        err = np.abs(g - r).max(axis=1) / _rowmax(ref[k][:n]) if g.size else np.zeros(n)
        worst[k] = float(err.max())
    print(f'{env_id} {tag} n={n}: worst error / max(1, |row|): ' + ', '.join(f'{k} {v:.2g}' for k, v in worst.items()))
    for k in KEYS:
        assert worst[k] <= BOUND, (k, worst[k])


@pytest.mark.parametrize('n', [1, 17, 33])
@pytest.mark.parametrize('env_id', MODELS)
def test_against_yardstick(env_id, n):
    c = _case(env_id)
    assert np.abs(c.u).max(axis=1).min() > 0.1 and np.abs(c.a).max(axis=1).min() > 1.0     # far from rest
    if n == NS:
        got = c.out
    else:
        got = {k: _np(v) for k, v in c.bk.eval(c.q[:n], c.u[:n], c.a[:n], points=c.pts, want=KEYS).items()}
    _compare(env_id, got, c.ref, n, 'ground')
    assert np.array_equal(got['point'][:, 1, 0], np.tile(c.pts[1][1], (n, 1))) and not got['point'][:, 1, 1:].any()
    assert [b for b, _ in c.pts].count('calcn_r') >= 2


@pytest.mark.parametrize('env_id', MODELS)
def test_local_frame(env_id):
    """BIOIM_BK_LOCAL: the velocities and accelerations of origin, com and
    orient in the body's own frame; everything else as without the flag."""
    c = _case(env_id)
    res = c.bk.eval(c.q, c.u, c.a, points=c.pts, local=True, want=KEYS)
    got = {k: _np(v) for k, v in res.items()}
    assert res.local and res.bodies == c.ys.bodies
    _compare(env_id, got, c.ref_local, NS, 'local')
    for k in ('rot', 'system', 'momentum', 'energy', 'point'):
        assert np.array_equal(got[k], c.out[k]), k
    for k in ('origin', 'com', 'orient'):
        assert np.array_equal(got[k][:, :, 0], c.out[k][:, :, 0]), k
        # (a planar model's angular velocity lies along z, the axis its bodies turn about: the same in both frames)
        assert k == 'orient' and env_id in (W2D, TLK2D) or np.abs(got[k][:, :, 1:] - c.out[k][:, :, 1:]).max() > 1e-3, k


@pytest.mark.parametrize('env_id', MODELS)
def test_identities(env_id):
    import torch
    from bioimitation.inverse_dynamics import MULT_M, InverseDynamics
    c = _case(env_id)
    ys, o = c.ys, c.out
    # a point at a body's origin / own mass centre is that row: one piece of code on the same numbers
    assert c.pts[6] == ('tibia_l', (0.0, 0.0, 0.0)) and c.pts[7][0] == 'femur_r'
    assert torch.equal(c.out_t['point'][:, 6], c.out_t['origin'][:, ys.bodies.index('tibia_l')])
    assert torch.equal(c.out_t['point'][:, 7], c.out_t['com'][:, ys.bodies.index('femur_r')])
    # None is zeros, bit for bit
    z = np.zeros_like(c.q)
    for kw_none, kw_zero in ((dict(u=c.u), dict(u=c.u, qdd=z)), (dict(qdd=c.a), dict(u=z, qdd=c.a)), ({}, dict(u=z, qdd=z))):
        x, y = (c.bk.eval(c.q, points=c.pts, want=KEYS, **kw) for kw in (kw_none, kw_zero))
        for k in KEYS:
            assert torch.equal(x[k], y[k]), (k, sorted(kw_none))
    # at rest: no velocity, no acceleration, no momentum, no kinetic energy
    assert not _np(x['origin'])[:, :, 1:].any() and not _np(x['momentum']).any() and not _np(x['energy'])[:, 0].any()
    # linear momentum is mass x the mass centre's velocity
    m = ys.mass.sum()
    e_p = np.abs(o['momentum'][:, 0] - m * o['system'][:, 1]).max(axis=1) / _rowmax(o['momentum'][:, 0])
    # kinetic energy is u . (M u) / 2
    idy = InverseDynamics(env_id)
    mu = _np(idy.eval(MULT_M, c.q, v=c.u))
    idy.close()
    ke = 0.5 * (c.u * mu).sum(axis=1)
    e_k = np.abs(o['energy'][:, 0] - ke) / np.maximum(1.0, ke)
    # rot is a rotation, and the angles are its body-fixed XYZ angles
    R = o['rot'].reshape(NS, ys.nos, 3, 3)
    e_r = np.abs(R @ R.transpose(0, 1, 3, 2) - np.eye(3)).max()
    a, b, g = (o['orient'][:, :, 0, i] for i in range(3))
    ca, sa, cb, sb, cg, sg = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(g), np.sin(g)
    one, zero = np.ones_like(a), np.zeros_like(a)
    mat = lambda rows: np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)  # noqa: E731
    Rx = mat([[one, zero, zero], [zero, ca, -sa], [zero, sa, ca]])
    Ry = mat([[cb, zero, sb], [zero, one, zero], [-sb, zero, cb]])
    Rz = mat([[cg, -sg, zero], [sg, cg, zero], [zero, zero, one]])
    e_a = np.abs(Rx @ Ry @ Rz - R).max()
    print(f'{env_id}: momentum vs m V {e_p.max():.2g} (bound {8 * EPS:.2g}), KE vs u.Mu/2 {e_k.max():.2g} (1e-12), '
          f'R R^T - 1 {e_r:.2g} (1e-14), angles -> R {e_a:.2g} (1e-13); KE {ke.min():.3g} .. {ke.max():.3g} J')
    assert e_p.max() <= 8 * EPS and e_k.max() <= 1e-12 and e_r <= 1e-14 and e_a <= 1e-13


def test_chain_rule():
    """Independent of the oracle: on Running3D the central difference of the
    positions along q +- h u gives the velocities, and that of the velocities
    along (q +- h u, u +- h q'') the accelerations (the angular velocity's
    gives the angular acceleration)."""
    c = _case(R3D)
    h = 1e-6
    keys = ('origin', 'com', 'orient', 'system', 'point')
    hi, lo = (c.bk.eval(c.q + s * h * c.u, c.u + s * h * c.a, points=c.pts, want=keys) for s in (1.0, -1.0))
    worst = 0.0
    for k in keys:
        d = (_np(hi[k]) - _np(lo[k])) / (2 * h)
        x = c.out[k]
        pairs = [(d[..., 1, :], x[..., 2, :])]                 # d(velocity) = acceleration
        if k != 'orient':
            pairs.append((d[..., 0, :], x[..., 1, :]))         # d(position) = velocity
        for dd, xx in pairs:
            err = (np.abs(dd - xx).reshape(NS, -1).max(axis=1) / _rowmax(xx)).max()
            worst = max(worst, err)
            assert err <= 1e-6, (k, err)
    print(f'{R3D}: chain rule, worst difference / max(1, |row|) {worst:.2g} (bound 1e-6)')


@pytest.mark.parametrize('env_id', [W2D, R3D])
def test_batch_independence_and_corners(env_id):
    import torch
    c = _case(env_id)
    again = c.bk.eval(c.q, c.u, c.a, points=c.pts, want=KEYS)
    for k in KEYS:
        assert torch.equal(again[k], c.out_t[k]), k              # a repeated call repeats
    for i in (0, 16, 32):                                         # a state alone is its row of the larger call
        one = c.bk.eval(c.q[i:i + 1], c.u[i:i + 1], c.a[i:i + 1], points=c.pts, want=KEYS)
        for k in KEYS:
            assert torch.equal(one[k][0], c.out_t[k][i]), (k, i)
    # npt = 0 and 1: the other outputs do not move, the one point is its row of the 19
    none = c.bk.eval(c.q, c.u, c.a, want=KEYS)
    assert none['point'].shape == (NS, 0, 3, 3)
    solo = c.bk.eval(c.q, c.u, c.a, points=c.pts[:1], want=KEYS)
    assert torch.equal(solo['point'][:, 0], c.out_t['point'][:, 0])
    for k in KEYS[:-1]:
        assert torch.equal(none[k], c.out_t[k]) and torch.equal(solo[k], c.out_t[k]), k
    assert c.bk.eval(c.q, want=('point',))['point'].numel() == 0      # nothing to compute: no launch
    # n = 0 is a no-op; a NaN in simply comes out
    empty = c.bk.eval(c.q[:0], points=c.pts, want=KEYS)
    assert empty['com'].shape == (0, c.ys.nos, 3, 3) and empty['point'].shape == (0, 19, 3, 3)
    q = c.q[:2].copy()
    q[1, 0] = np.nan
    bad = _np(c.bk.eval(q, c.u[:2], c.a[:2], want=('system',))['system'])
    assert np.isnan(bad[1]).any() and np.array_equal(bad[0], c.out['system'][0])
    # the entry point's own refusals, before any launch
    import ctypes as C
    from bioimitation import _lib
    env = c.bk._env
    qt = torch.as_tensor(c.q[:1], device=env.device)
    out = torch.empty((1, 3, 3), dtype=env.dtype, device=env.device)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    body = (C.c_int32 * 2)(0, c.ys.nos)
    loc = (C.c_double * 6)()
    nul = [None] * 8

    def call(n, q, npt, pb, pl, flags, outs):
        return env._L.bioim_body_kin(env._h, n, q, None, None, npt, pb, pl, flags, *outs)
    sysout = nul[:4] + [vp(out)] + nul[5:]
    for args, msg in (((-1, vp(qt), 0, None, None, 0, sysout), b'negative n'),
                      ((1, vp(qt), -1, None, None, 0, sysout), b'npt must be in'),
                      ((1, vp(qt), 65, body, loc, 0, sysout), b'npt must be in'),
                      ((1, vp(qt), 2, None, loc, 0, sysout), b'null point table'),
                      ((1, vp(qt), 2, body, loc, 0, sysout), b'outside [-1, nosbody)'),
                      ((1, vp(qt), 0, None, None, 2, sysout), b'unknown flag bits'),
                      ((1, None, 0, None, None, 0, sysout), b'null q'),
                      ((1, vp(qt), 0, None, None, 0, nul), b'no output requested')):
        assert call(*args) < 0
        err = _lib.load().bioim_last_error()
        assert err.startswith(b'bioim_body_kin:') and msg in err, (msg, err)
    assert call(0, None, 0, None, None, 0, sysout) == 0


def test_fp32_against_fp64():
    """An fp32 handle on Walking2D, n = 17, against the fp64 result."""
    from bioimitation.body_kinematics import BodyKinematics
    c = _case(W2D)
    n = 17
    bk32 = BodyKinematics(W2D, precision=32)
    res = bk32.eval(c.q[:n], c.u[:n], c.a[:n], points=c.pts, want=KEYS)
    bk32.close()
    worst = {}
    for k in KEYS:
        import torch
        assert res[k].dtype == torch.float32
        g, r = _np(res[k]).reshape(n, -1), c.out[k][:n].reshape(n, -1)
        worst[k] = float((np.abs(g - r).max(axis=1) / _rowmax(c.out[k][:n])).max())
    w = max(worst.values())
    print(f'{W2D} fp32 vs fp64, n={n}: worst error / max(1, |row|) {w:.3g} (recorded {FP32_OBSERVED:.3g}, bound '
          f'{4 * FP32_OBSERVED:.3g}): ' + ', '.join(f'{k} {v:.2g}' for k, v in worst.items()))
    assert w <= 4 * FP32_OBSERVED


@pytest.mark.parametrize('env_id', [W2D, R3D])
def test_env_body_kinematics(env_id, tmp_path):
    """VectorEnv.body_kinematics on 4 envs after 5 steps: equal to
    BodyKinematics.eval on the state rows' q and u bit for bit, and a read: a
    twin env that is not asked steps on bit-identically for three steps and
    has the same cache_ok plane."""
    import torch
    from bioimitation import storage
    from bioimitation.packdef import state_row_slices
    from bioimitation.vector_env import VectorEnv
    c = _case(env_id)
    n = 4
    a, b = (VectorEnv(env_id, n, precision=64, seed=3) for _ in range(2))
    pk = a.pack
    acts = torch.as_tensor(np.random.default_rng(32).uniform(0, 1, size=(8, n, a.action_dim)), device=a.device)
    for e in (a, b):
        e.reset(ref_index=[4, 20, 36, 52])
        for t in range(5):
            e.step(acts[t])
    pts = c.pts[:3]
    got = a.body_kinematics(points=pts, want=KEYS)
    part = a.body_kinematics(env_ids=[2, 0], points=pts, local=True, want=('com', 'point'))
    assert got.bodies == c.ys.bodies and not got.local and part.local
    assert torch.equal(part['point'], got['point'][[2, 0]])
    assert np.array_equal(a.debug_plane('cache_ok'), b.debug_plane('cache_ok'))
    rows = a.state_rows()
    sl, _ = state_row_slices(pk.ndof, pk.nmuscle, pk.nact, pk.horizon)
    q, u = rows[:, sl['q']], rows[:, sl['u']]
    want = c.bk.eval(q, u, points=pts, want=KEYS)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    files = c.bk.write_sto(str(tmp_path), 0.01 * np.arange(n), a.body_kinematics(want=('com', 'orient', 'system')))
    assert [f.rsplit('_', 2)[-2] for f in files] == ['pos', 'vel', 'acc']
    assert storage.read_sto(files[0])[2].shape == (n, 1 + 6 * pk.nosbody + 3)
    for t in range(5, 8):
        ra, rb = a.step(acts[t]), b.step(acts[t])
        for x, y, what in zip(ra, rb, ('obs', 'reward', 'done', 'info')):
            assert torch.equal(x, y), (what, t)
        assert np.array_equal(a.debug_plane('cache_ok'), b.debug_plane('cache_ok'))
    # qdd='own': with the envs' forward-dynamics q'' the mass centre's acceleration is the REALIZE report's
    own, rest = a.body_kinematics(qdd='own', want=('system',)), a.body_kinematics(want=('system',))
    k0 = 2 + 3 * pk.ncoord + 18 * pk.nosbody
    acc = a.osim_report[:, k0 + 6:k0 + 9]
    assert torch.equal(own['system'][:, :2], rest['system'][:, :2])
    assert (own['system'][:, 2] - acc).abs().max().item() <= BOUND * max(1.0, acc.abs().max().item())
    a.close()
    b.close()
