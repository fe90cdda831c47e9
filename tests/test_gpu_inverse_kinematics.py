"""Batched marker inverse kinematics (bioim_ik_solve,
bioimitation.inverse_kinematics) against the oracle's forward kinematics and
the CPU yardstick of tests/ik_reference.py (validated by
tests/test_ik_reference.py).

Frames: evaluate-only on every frame of the two shipped IK trials (182 / 239);
the solves on every 6th frame (31 / 40 frames: two workgroups each, the second
partial), the yardstick's own choice; the synthetic problems with n = 1, 17
(a second workgroup with one frame) and 64.  The yardstick's solutions are
computed once per session and shared.

Bounds:
- markers, err at a given q: 1e-12 (metres; rounding of a chain of 7 frames at
  coordinates of a few metres is ~1e-15);
- jacobian: 1e-7 per entry against central differences (h = 1e-6) of the
  oracle FK, 100 x the eps |x| / h ~ 1e-9 round-off of the difference quotient;
  exact 0 off the root chain;
- synthetic recovery: |q - q*| <= 1e-8 at tol 1e-10, status in [1, 50];
- the shipped trials: |q - q_yardstick| <= 1e-7 = 100 tol (a step-size stop at
  tol leaves each solver within rho / (1 - rho) tol <= 20 tol of the minimizer
  for a linear rate rho <= 0.95), and the yardstick's Gauss-Newton step at the
  GPU's q <= max(10 tol, 10 x the yardstick's own floor).
Observed maxima and iteration ranges are printed (DESIGN.md 5.16 lists them).

One case differs from its first statement: a 17-marker problem cannot hold the
trial's 28 markers, so the nm = 17 corner cycles a 14-marker subset (every
second marker, which still spans every body) and is compared with the
14-marker solve, itself compared with the yardstick; nm = 64 cycles all 28 and
is compared with the 28-marker solve.
"""
import numpy as np
import pytest

import ik_reference as R
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason='needs GPU')]

TRIALS = ['3D', '02905']
TOL = R.TOL
W2D, K3D = 'MuscleWalkingImitation2D-v0', 'MuscleLockedKneeImitation3D-v0'
KEYS = ('q', 'markers', 'err', 'jacobian', 'status')


def _np(t):
    return t.double().cpu().numpy() if t.dtype.is_floating_point else t.cpu().numpy()


@pytest.fixture(scope='module')
def solvers():
    """one InverseKinematics per (ID, marker list), shared by the module's tests"""
    from bioimitation.inverse_kinematics import InverseKinematics
    made = {}

    def get(mm, sub=None):
        key = (mm.env_id, mm.nm, None if sub is None else tuple(sub))
        if key not in made:
            pairs = mm.pairs()
            made[key] = InverseKinematics(mm.env_id, pairs if sub is None else [pairs[i] for i in sub])
        return made[key]
    yield get
    for s in made.values():
        s.close()


@pytest.mark.parametrize('tag', TRIALS)
def test_evaluate_matches_oracle_fk(tag, solvers, oracle_lib):
    z, mm = R.trial_model(oracle_lib, tag)
    ik = solvers(mm)
    q = np.array([mm.qdof(qc) for qc in z['q']])
    x, w = z['x_exp'], z['weights']
    out = ik.evaluate(q, x, w, want=('markers', 'err', 'q', 'status'))
    ref = np.array([mm.markers(qf) for qf in q])
    ref_err = np.array([R.marker_err(ref[f], x[f], w) for f in range(len(q))])
    em, ee = np.abs(_np(out['markers']) - ref).max(), np.abs(_np(out['err']) - ref_err).max()
    print(f'{tag}: {len(q)} frames, markers {em:.2e}, err {ee:.2e}; RMS median {np.median(ref_err[:, 0]) * 1e3:.1f} mm')
    assert em <= 1e-12 and ee <= 1e-12
    assert (_np(out['q']) == q).all() and (_np(out['status']) == 0).all()


def _jacobian_cases(oracle_lib):
    for tag in TRIALS:
        z, mm = R.trial_model(oracle_lib, tag)
        fr = np.linspace(0, len(z['q']) - 1, 16).astype(int)
        yield tag, mm, np.array([mm.qdof(z['q'][f]) for f in fr])
    for env_id in (W2D, K3D):
        mm, _, qstar = R.synthetic_model(oracle_lib, env_id)
        yield env_id, mm, qstar[::4]


def test_jacobian_matches_central_differences(solvers, oracle_lib):
    for name, mm, q in _jacobian_cases(oracle_lib):
        J = _np(solvers(mm).evaluate(q, want=('jacobian',))['jacobian'])
        assert J.shape == (16, mm.nm, 3, mm.ndof)
        ref = np.array([mm.jacobian(qf) for qf in q])
        on = mm.chain_mask()
        off = np.broadcast_to(~on[None, :, None, :], J.shape)
        err = np.abs(J - ref).max()
        print(f'{name}: jacobian vs central differences {err:.2e}; {off[0].sum()} exact zeros per frame')
        assert err <= 1e-7
        assert (J[off] == 0).all() and off.any()
        assert (np.abs(J).max(axis=(0, 2))[on] > 0).mean() > 0.9      # (a marker on a joint axis may not move)


@pytest.mark.parametrize('n', [1, 17, 64])
@pytest.mark.parametrize('env_id', R.SYNTHETIC)
def test_synthetic_recovery(env_id, n, solvers, oracle_lib):
    mm, w, qstar = R.synthetic_model(oracle_lib, env_id)
    qs = qstar[:n]
    x = np.array([mm.markers(q) for q in qs])
    q0 = R.synthetic_start(mm, qs, 100 + n)
    out = solvers(mm).solve(x, w, q0, tol=1e-10, max_iter=50, want=KEYS)
    q, st = _np(out['q']), _np(out['status'])
    print(f'{env_id} n={n}: recovery {np.abs(q - qs).max():.2e}, iterations {st.min()}-{st.max()}, '
          f'marker rms {_np(out["err"])[:, 0].max():.2e}')
    assert (st >= 1).all() and (st <= 50).all()
    assert np.abs(q - qs).max() <= 1e-8
    assert np.abs(_np(out['markers']) - x).max() <= 1e-8 * 10      # |dx| <= |J| |dq|, |J| columns <= ~2 m / rad


@pytest.mark.parametrize('tag,start', [('3D', 'warm'), ('3D', 'cold'), ('02905', 'warm')])
def test_shipped_trials_against_the_yardstick(tag, start, solvers, oracle_lib):
    z, mm = R.trial_model(oracle_lib, tag)
    sol = R.trial_solution(oracle_lib, tag, start)
    floor = R.noise_floor(oracle_lib, tag)
    fr, w = sol['frames'], z['weights']
    x = z['x_exp'][fr]
    out = solvers(mm).solve(x, w, sol['q0'] if start == 'warm' else None, tol=TOL, max_iter=R.CAPS[tag],
                            want=('q', 'status', 'err'))
    q, st = _np(out['q']), _np(out['status'])
    ok = sol['status'] >= 0
    dist = np.abs(q - sol['q'])[ok].max()
    gn = max(R.gauss_newton_step(mm, q[k], x[k], w) for k in range(len(fr)) if ok[k])
    print(f'{tag} {start}: {len(fr)} frames, |q - yardstick| {dist:.2e}, Gauss-Newton step at q {gn:.2e} '
          f'(floor {floor:.2e}); iterations GPU {st[st >= 0].min()}-{st[st >= 0].max()} (mean {st[st >= 0].mean():.1f}), '
          f'yardstick {sol["status"][ok].min()}-{sol["status"][ok].max()}; RMS median '
          f'{np.median(_np(out["err"])[:, 0]) * 1e3:.1f} mm')
    assert ((st >= 0) == ok).all()
    assert dist <= 100 * TOL
    assert gn <= max(10 * TOL, 10 * floor)


def _trial_problem(oracle_lib, k=8):
    """the first k solve frames of the 3D trial: (mm, x, w, warm q0, the yardstick's q)"""
    z, mm = R.trial_model(oracle_lib, '3D')
    sol = R.trial_solution(oracle_lib, '3D', 'warm')
    fr = sol['frames'][:k]
    return mm, z['x_exp'][fr], z['weights'], sol['q0'][:k], sol['q'][:k]


def test_one_marker_with_coordinate_tasks(solvers, oracle_lib):
    mm, x, w, q0, _ = _trial_problem(oracle_lib, 4)
    sub = [6]      # RKNE
    m1 = R.MarkerModel(oracle_lib, mm.env_id, [mm.names['bodies'][mm.bidx[6]]], mm.L[sub])
    cw = np.full(mm.ndof, 0.5)
    qt = q0 + 0.05
    out = solvers(mm, sub).solve(x[:, sub], w[sub], q0, cw, qt, tol=TOL, max_iter=200, want=('q', 'status'))
    q, st = _np(out['q']), _np(out['status'])
    ref = [R.solve(m1, x[k][sub], w[sub], q0[k], cw, qt[k], tol=TOL, max_iter=200) for k in range(len(x))]
    d = max(np.abs(q[k] - ref[k][0]).max() for k in range(len(x)))
    print(f'one marker + coordinate tasks: |q - yardstick| {d:.2e}, iterations {st.min()}-{st.max()}')
    assert (st >= 1).all() and all(r[1] >= 1 for r in ref)
    assert d <= 100 * TOL


@pytest.mark.parametrize('nm', [17, 64])
def test_cycled_markers_leave_the_solution(nm, solvers, oracle_lib):
    """markers repeated with their weight split: the same objective, the same q"""
    mm, x, w, q0, qy = _trial_problem(oracle_lib)
    base = list(range(0, mm.nm, 2)) if nm < mm.nm else list(range(mm.nm))
    cyc = [base[i % len(base)] for i in range(nm)]
    count = np.bincount(cyc, minlength=mm.nm)
    want = ('q', 'status', 'err')
    a = solvers(mm, base).solve(x[:, base], w[base], q0, tol=TOL, want=want)
    b = solvers(mm, cyc).solve(x[:, cyc], (w / np.maximum(count, 1))[cyc], q0, tol=TOL, want=want)
    d = np.abs(_np(a['q']) - _np(b['q'])).max()
    print(f'nm={nm} from {len(base)} markers: |q - q_base| {d:.2e}, iterations {_np(b["status"]).min()}-'
          f'{_np(b["status"]).max()}')
    assert (_np(a['status']) >= 1).all() and (_np(b['status']) >= 1).all()
    assert d <= 100 * TOL
    assert np.abs(_np(a['err'])[:, 0] - _np(b['err'])[:, 0]).max() <= 1e-9      # the weighted RMS is the same sum
    if nm >= mm.nm:
        assert np.abs(_np(a['q']) - qy).max() <= 100 * TOL
    else:      # the subset's own yardstick
        ms = R.MarkerModel(oracle_lib, mm.env_id, [mm.names['bodies'][b_] for b_ in mm.bidx[base]], mm.L[base])
        ref = np.array([R.solve(ms, x[k][base], w[base], q0[k], tol=TOL)[0] for k in range(len(x))])
        assert np.abs(_np(a['q']) - ref).max() <= 100 * TOL


def test_nan_marker_is_a_zero_weight(solvers, oracle_lib):
    import torch
    mm, x, w, q0, _ = _trial_problem(oracle_lib)
    ik = solvers(mm)
    gap, frames = 9, [1, 4, 5]      # RHEE
    xn = x.copy()
    xn[frames, gap, 1] = np.nan
    xn[frames[0], gap] = np.nan
    full = ik.solve(x, w, q0, tol=TOL, want=KEYS)
    got = ik.solve(xn, w, q0, tol=TOL, want=KEYS)
    w0 = w.copy()
    w0[gap] = 0.0
    for k in range(len(x)):
        if k in frames:
            ref = ik.solve(x[k:k + 1], w0, q0[k:k + 1], tol=TOL, want=KEYS)
            for key in KEYS:
                assert torch.equal(got[key][k], ref[key][0]), (k, key)
            assert not torch.equal(got['q'][k], full['q'][k])
        else:
            for key in KEYS:
                assert torch.equal(got[key][k], full[key][k]), (k, key)
    assert (_np(got['status']) >= 1).all()


def test_iteration_cap_and_empty_frames(solvers, oracle_lib):
    """max_iter = 1: status -1 with an accepted iterate (the objective went
    down).  A frame whose markers are all gaps, without coordinate tasks, has
    A = 0: status -2, q = q0, the outputs still written, the other frames
    untouched; with coordinate tasks it goes to the target."""
    import torch
    mm, x, w, q0, _ = _trial_problem(oracle_lib)
    ik = solvers(mm)
    q0 = q0 + 0.01
    at0 = _np(ik.evaluate(q0, x, w, want=('err',))['err'])
    one = ik.solve(x, w, q0, tol=TOL, max_iter=1, want=KEYS)
    assert (_np(one['status']) == -1).all()
    assert (_np(one['err'])[:, 0] < at0[:, 0]).all() and (np.abs(_np(one['q']) - q0).max(axis=1) > 0).all()
    xe = x.copy()
    xe[2] = np.nan
    full = ik.solve(x, w, q0, tol=TOL, want=KEYS)
    got = ik.solve(xe, w, q0, tol=TOL, want=KEYS)
    st = _np(got['status'])
    assert st[2] == -2 and (np.delete(st, 2) >= 1).all()
    assert (_np(got['q'])[2] == q0[2]).all() and (_np(got['err'])[2] == 0).all()
    assert np.isfinite(_np(got['markers'])).all() and np.isfinite(_np(got['jacobian'])).all()
    for k in (0, 1, 3, 7):
        for key in KEYS:
            assert torch.equal(got[key][k], full[key][k]), (k, key)
    cw, qt = np.ones(mm.ndof), q0 - 0.02
    tasks = ik.solve(xe, w, q0, cw, qt, tol=TOL, want=('q', 'status'))
    assert _np(tasks['status'])[2] >= 1 and np.abs(_np(tasks['q'])[2] - qt[2]).max() <= 1e-12
    # a NaN start is a NaN that came in
    qn = q0.copy()
    qn[5, 3] = np.nan
    bad = ik.solve(x, w, qn, tol=TOL, want=('q', 'status'))
    assert _np(bad['status'])[5] == -2 and (np.delete(_np(bad['status']), 5) >= 1).all()


def test_frames_are_independent_and_calls_repeat(solvers, oracle_lib):
    import torch
    z, mm = R.trial_model(oracle_lib, '3D')
    sol = R.trial_solution(oracle_lib, '3D', 'warm')
    ik = solvers(mm)
    x, w, q0 = z['x_exp'][sol['frames']], z['weights'], sol['q0']
    full = ik.solve(x, w, q0, tol=TOL, want=KEYS)
    again = ik.solve(x, w, q0, tol=TOL, want=KEYS)
    for key in KEYS:
        assert torch.equal(full[key], again[key]), key
    for i in (0, 15, 16, 30):
        one = ik.solve(x[i:i + 1], w, q0[i:i + 1], tol=TOL, want=KEYS)
        for key in KEYS:
            assert torch.equal(one[key][0], full[key][i]), (i, key)


def test_a_solve_between_steps_is_a_read(oracle_lib):
    """Twin envs; one carries a handle that also solves IK between steps (the
    handle of InverseKinematics is a VectorEnv's, so the call runs on an env
    that steps): the next three steps agree bit for bit and the realize-cache
    flags do not move (the check of test_gpu_static_opt.py)."""
    import ctypes as C
    import torch
    from bioimitation import _lib
    from bioimitation.vector_env import VectorEnv
    mm, w, qstar = R.synthetic_model(oracle_lib, W2D)
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
    from bioimitation.inverse_kinematics import map_markers
    _, cb, loc = map_markers(a.pack, mm.names['bodies'], mm.pairs())
    dev = lambda v, dt=torch.float64: torch.as_tensor(v, device=a.device, dtype=dt).contiguous()  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    nf = 20
    x = dev(np.array([mm.markers(q) for q in qstar[:nf]]))
    q0 = dev(R.synthetic_start(mm, qstar[:nf], 3))
    cbd, locd, wd = dev(cb, torch.int32), dev(loc), dev(w)
    q, st = torch.empty_like(q0), torch.empty(nf, dtype=torch.int32, device=a.device)
    a._bind_stream()
    _lib.check(a._L.bioim_ik_solve(a._h, nf, mm.nm, p(cbd), p(locd), p(wd), p(x), p(q0), None, None, 1e-10, 50,
                                   p(q), None, None, None, p(st)))
    assert (_np(st) >= 1).all() and np.abs(_np(q) - qstar[:nf]).max() <= 1e-8
    assert (a.debug_plane('cache_ok') == flags).all()
    assert (b.debug_plane('cache_ok') == flags).all()
    for t in (2, 3, 4):
        ra, rb = a.step(acts[t]), b.step(acts[t])
        for u, v, what in zip(ra, rb, ('obs', 'reward', 'done', 'info')):
            assert torch.equal(u, v), (t, what)
    assert (a.debug_plane('cache_ok') == b.debug_plane('cache_ok')).all()
    a.close()
    b.close()


def test_refusals_and_trc(solvers, oracle_lib, tmp_path):
    """The library's last refusal (fp64 handles only) on a real fp32 handle;
    solve_trc on a file written from synthetic markers returns the motion."""
    import ctypes as C
    import torch
    from bioimitation.vector_env import VectorEnv
    env = VectorEnv(W2D, 2, precision=32)
    t = torch.zeros((2, 64), dtype=torch.float64, device=env.device)
    p = C.c_void_p(t.data_ptr())
    assert env._L.bioim_ik_solve(env._h, 2, 1, p, p, p, p, p, None, None, 1e-9, 10, p, None, None, None, None) == -1
    err = env._L.bioim_last_error()
    assert err.startswith(b'bioim_ik_solve:') and b'fp64 handles only' in err, err
    env.close()
    mm, w, qstar = R.synthetic_model(oracle_lib, W2D)
    ik = solvers(mm)
    qs = qstar[:5]
    X = np.array([mm.markers(q) for q in qs])
    path = tmp_path / 'synthetic.trc'
    names = ik.marker_names
    lines = ['PathFileType\t4\t(X/Y/Z)\tsynthetic.trc',
             'DataRate\tCameraRate\tNumFrames\tNumMarkers\tUnits', f'100\t100\t{len(qs)}\t{len(names)}\tmm',
             'Frame#\tTime\t' + '\t\t\t'.join(names) + '\t\t',
             '\t\t' + '\t'.join(f'X{i + 1}\tY{i + 1}\tZ{i + 1}' for i in range(len(names))), '']
    for f in range(len(qs)):
        lines.append(f'{f + 1}\t{f * 0.01:.2f}\t' + '\t'.join(f'{v * 1e3:.9f}' for v in X[f].ravel()))
    path.write_text('\n'.join(lines) + '\n')
    time, qc, out = ik.solve_trc(str(path), {names[0]: 2.0}, q0=R.synthetic_start(mm, qs, 9), tol=1e-10)
    assert np.allclose(time, np.arange(5) * 0.01) and qc.shape == (5, mm.ncoord)
    assert (_np(out['status']) >= 1).all()
    assert np.abs(np.array([mm.qdof(r) for r in qc]) - qs).max() <= 1e-8      # the file keeps 1e-12 m
    from bioimitation.storage import read_sto
    ik.write_mot(str(tmp_path / 'ik.mot'), time, qc)
    hdr, labels, data = read_sto(str(tmp_path / 'ik.mot'))
    assert hdr['inDegrees'] == 'no' and labels == ['time'] + ik.coordinate_names
    assert np.abs(data - np.column_stack([time, qc])).max() <= 1e-10      # write_sto keeps 10 decimals
