"""Batched induced accelerations (bioim_induced_accel,
bioimitation.induced_accelerations, VectorEnv.induced_accelerations) on the
GPU.

States: tests/ia_reference.py::draw_cases, 8 per model, strictly inside every
limited coordinate's range, u != 0, state 0 with a foot in Hunt-Crossley
contact; tendon forces from bioim_muscle_eval at activations U(0.05, 1);
tau_act and ext random.  The held feet of the explicit POINT call cycle through
flight, left, right and double stance (cactive / cpoint given: a foot sphere's
centre); one test per model takes the model's own decision instead.  Models:
Walking2D (planar, moving points), Running3D, LockedKnee3D (merged leg),
TorqueLockedKnee2D (no muscles).

Bounds.
  Against the yardstick (tests/ia_reference.py: dense KKT solves from the
  oracle's M, g, c, dL/dq and contact, J / beta / J_com from differentiated
  poses): accel, com_accel and reaction within 10x the yardstick's own
  h-vs-h/2 noise of that state and output.
  Exact identities: 1e-9 x the state's sum of |terms| (for an identity between
  accelerations the sum of |A_c| over all columns, for the momentum identity
  the forces that enter it).
Observed values are printed."""
import functools

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason='needs GPU')]

W2D, R3D, LK3D, TLK2D = ('MuscleWalkingImitation2D-v0', 'MuscleRunningImitation3D-v0',
                         'MuscleLockedKneeImitation3D-v0', 'TorqueLockedKneeImitation2D-v0')
MODELS = [W2D, R3D, LK3D, TLK2D]
NS = 8
KEYS = ('accel', 'com_accel', 'reaction', 'cpoint', 'cactive', 'status')
GRAVITY, CORIOLIS, MULT_M, MULT_MINV, RESIDUAL = 0, 1, 2, 3, 4
OWN_THRESHOLD = 1.0      # N, the `own` call's force_threshold


def _np(t):
    return t.double().cpu().numpy() if t.is_floating_point() else t.cpu().numpy()


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(env_id):
    """The model's solver objects, test states and the two calls' outputs
    (computed once, shared, read-only)."""
    import oracle
    import ia_reference as R
    from bioimitation.induced_accelerations import InducedAccelerations
    from bioimitation.inverse_dynamics import InverseDynamics
    from bioimitation.muscle_analysis import MuscleAnalysis
    c = Case()
    c.ys = R.yardstick(oracle, env_id)
    c.ia = InducedAccelerations(env_id)
    c.id = InverseDynamics(env_id)
    c.q, c.u, c.tau_act, c.ext, c.cactive, c.cpoint = R.draw_cases(c.ys, NS, seed=31)
    c.nm, c.nf, c.nd = c.ys.nm, c.ys.nf, c.ys.nd
    c.ft = c.mtau = None
    if c.nm:
        ma = MuscleAnalysis(env_id)
        act = np.random.default_rng(32).uniform(0.05, 1.0, size=(NS, c.nm))
        r = ma.eval(c.q, c.u, act=act, want=('fiber', 'tau'))
        c.ft, c.mtau = _np(r['fiber'])[:, :, 2].copy(), _np(r['tau'])
        ma.close()
    ev = lambda **kw: {k: _np(v) for k, v in c.ia.eval(c.q, c.u, c.ft, c.tau_act, c.ext, want=KEYS, **kw).items()}  # noqa: E731
    c.force = ev(kind='force')
    c.point = ev(kind='point', cactive=c.cactive, cpoint=c.cpoint)
    c.own = ev(kind='point', force_threshold=OWN_THRESHOLD)
    for a in vars(c).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _ref(env_id, kind, i):
    """The yardstick's values of state i: 'force', 'point' (the explicit feet)
    or 'own' (the feet and points of the yardstick's own restatement of the
    model's decision, at the threshold of the `own` call)."""
    c = _case(env_id)
    kw = {}
    if kind == 'point':
        kw = dict(cactive=c.cactive[i], cpoint=c.cpoint[i])
    elif kind == 'own':
        fs, P, _, _ = c.ys.own_feet(c.q[i], c.u[i])
        kw = dict(cactive=fs > OWN_THRESHOLD, cpoint=np.nan_to_num(P))
    return c.ys.eval(c.q[i], c.u[i], None if c.ft is None else c.ft[i], c.tau_act[i], c.ext[i],
                     kind='force' if kind == 'force' else 'point', **kw)


def _minv(c, rhs):
    return _np(c.id.eval(MULT_MINV, c.q, None, rhs))


@pytest.mark.parametrize('env_id', MODELS)
def test_against_yardstick(env_id):
    c = _case(env_id)
    worst = 0.0
    for i in range(NS):
        for kind, out in (('force', c.force), ('point', c.point), ('own', c.own)):
            r = _ref(env_id, kind, i)
            for k in ('accel', 'com_accel', 'reaction'):
                err, bound = np.abs(out[k][i] - r[k]).max(), 10.0 * r['noise'][k]
                ratio = err / bound if bound > 0 else (0.0 if err == 0 else np.inf)
                worst = max(worst, ratio)
                print(f'{env_id} state {i} {kind} {k}: max |value| {np.abs(r[k]).max():.3g} noise {r["noise"][k]:.2g} '
                      f'err {err:.2g} bound {bound:.2g}')
                assert err <= bound, (i, kind, k, err, bound)
    print(f'{env_id}: worst error / bound {worst:.3g}')


@pytest.mark.parametrize('env_id', MODELS)
def test_superposition_and_momentum(env_id):
    c = _case(env_id)
    ys = c.ys
    m, g = ys.mass.sum(), ys.g
    assert (c.force['status'] == 0).all() and (c.point['status'] == 0).all() and (c.own['status'] == 0).all()
    worst = dict(sum=0.0, momentum=0.0)
    for kind, out in (('force', c.force), ('point', c.point), ('own', c.own)):
        for i in range(NS):
            for k in ('accel', 'com_accel', 'reaction'):
                a = out[k][i]
                err, terms = np.abs(a[:-1].sum(0) - a[-1]).max(), np.abs(a[:-1]).sum()
                worst['sum'] = max(worst['sum'], err / max(terms, 1e-300))
                assert err <= 1e-9 * terms, (kind, i, k, err, terms)
            # m com_accel_c = sum_f reaction_{c,f} + [gravity] m g + [external] sum_k F_ext,k + [contact column] F_f
            rhs = out['reaction'][i].sum(1)
            rhs[0] += m * g
            rhs[4 + c.nf] += c.ext[i][:, :3].sum(0)
            _, w = ys.orc.contact(c.q[i], c.u[i])
            for f in range(c.nf):
                if not out['cactive'][i, f]:
                    rhs[2 + f] += w[6 * f:6 * f + 3]
            rhs[-1] = rhs[:-1].sum(0)
            lhs = m * out['com_accel'][i]
            terms = np.abs(out['reaction'][i]).sum() + m * np.abs(g).sum() + np.abs(c.ext[i][:, :3]).sum() + \
                np.abs(w).sum() + np.abs(lhs[:-1]).sum()
            err = np.abs(lhs - rhs)[:, :ys.nr].max()      # a planar model's root joint carries z
            worst['momentum'] = max(worst['momentum'], err / terms)
            assert err <= 1e-9 * terms, (kind, i, err, terms)
            if kind == 'force' and c.nm:   # a muscle alone does not move the mass centre
                assert np.abs(lhs[5 + c.nf:-1, :ys.nr]).max() <= 1e-9 * terms
        if kind != 'force' and env_id in (W2D, TLK2D):
            assert not out['reaction'][..., 2].any()          # the planar z: exactly 0
    assert not c.force['reaction'].any() and not c.force['cactive'].any()
    print(f'{env_id}: worst / terms {worst}')


@pytest.mark.parametrize('env_id', MODELS)
def test_force_identities(env_id):
    c = _case(env_id)
    A = c.force['accel']
    terms = np.abs(A[:, :-1]).sum((1, 2))
    grav = _minv(c, _np(c.id.eval(GRAVITY, c.q)))
    vel = _minv(c, -_np(c.id.eval(CORIOLIS, c.q, c.u)))
    worst = {}
    for name, got, ref in (('gravity', A[:, 0], grav), ('velocity', A[:, 1], vel)):
        err = np.abs(got - ref).max(1)
        worst[name] = (err / terms).max()
        assert (err <= 1e-9 * terms).all(), (name, err, terms)
    if c.nm:
        err = np.abs(A[:, 5 + c.nf:-1].sum(1) - _minv(c, c.mtau)).max(1)
        worst['muscles'] = (err / terms).max()
        assert (err <= 1e-9 * terms).all(), (err, terms)
    err = np.abs(A[:, 3 + c.nf] - _minv(c, c.tau_act)).max(1)
    worst['actuators'] = (err / terms).max()
    assert (err <= 1e-9 * terms).all(), (err, terms)
    # RESIDUAL(q, u, total) = the muscle + actuator + external generalized force.  The external one independently:
    # bioim_joint_reaction's tau_joint = S_d . F falls by exactly S_d . (ext on the bodies d moves) when ext is applied
    from bioimitation.joint_reaction import JointReaction
    jr = JointReaction(env_id)
    tj = [_np(jr.eval(c.q, c.u, None, c.ft, e, frame='ground', want=('tau_joint',))['tau_joint']) for e in (None, c.ext)]
    jr.close()
    qext = tj[0] - tj[1]
    assert (np.abs(qext).max(1) > 1.0).all()              # ext does act on every state
    err = np.abs(A[:, 4 + c.nf] - _minv(c, qext)).max(1)
    worst['external'] = (err / terms).max()
    assert (err <= 1e-9 * terms).all(), (err, terms)
    tot = A[:, -1]
    res = _np(c.id.eval(RESIDUAL, c.q, c.u, tot))
    rhs = c.tau_act + (c.mtau if c.nm else 0.0) + qext
    M = np.stack([np.abs(c.ys.orc.mass_bias(c.q[i], c.u[i])[0]) @ np.abs(tot[i]) for i in range(NS)])
    fterms = M.sum(1) + np.abs(rhs).sum(1) + np.abs(res).sum(1) + np.abs(tj[0]).sum(1) + np.abs(tj[1]).sum(1)
    err = np.abs(res - rhs).max(1)
    worst['residual'] = (err / fterms).max()
    assert (err <= 1e-9 * fterms).all(), (err, fterms)
    print(f'{env_id}: worst / terms {worst}')


@pytest.mark.parametrize('env_id', MODELS)
def test_point_constraints(env_id):
    """J A_c + [velocity or total] beta = 0, with J from bioim_ik_solve's jacobian
    at max_iter = 0, a marker on the foot's body at P_f.  Exactly (1e-9 of the
    terms): J A_c = 0 on every column but velocity and total, whose J A_c agree.
    beta is no output, so the velocity column takes the yardstick's (a second
    difference of the foot point along q + u t), within 10x its noise."""
    from bioimitation.inverse_kinematics import InverseKinematics
    from bioimitation.obslayout import load_names
    c = _case(env_id)
    ys = c.ys
    names = load_names(env_id)['bodies']
    nr = 2 if env_id in (W2D, TLK2D) else 3
    worst, worst_b = 0.0, 0.0
    for kind, out in (('point', c.point), ('own', c.own)):
        held = [(i, f) for i in range(NS) for f in range(c.nf) if out['cactive'][i, f]]
        assert held
        markers = []
        for i, f in held:
            R, p, _ = ys.orc.fk(c.q[i])
            ob = ys.first[ys.force_body[f]]
            markers.append((names[ob], R[ob].T @ (out['cpoint'][i, f] - p[ob])))
        ik = InverseKinematics(env_id, markers)
        J = _np(ik.evaluate(c.q, want=('jacobian',))['jacobian'])
        ik.close()
        for k, (i, f) in enumerate(held):
            A = out['accel'][i]
            JA = A @ J[i, k, :nr].T                       # [NC][nr]
            terms = np.abs(J[i, k, :nr]).sum() * np.abs(A[:-1]).sum()
            err = max(np.abs(np.delete(JA, [1, len(A) - 1], axis=0)).max(), np.abs(JA[1] - JA[-1]).max())
            worst = max(worst, err / terms)
            assert err <= 1e-9 * terms, (i, f, err, terms)
            r = _ref(env_id, kind, i)
            j = int(out['cactive'][i, :f].sum())            # f's place among the state's held feet
            beta, bound = r['beta'][nr * j:nr * j + nr], 10.0 * r['noise']['beta']
            assert r['beta'].size == nr * int(out['cactive'][i].sum())
            errb = max(np.abs(JA[1] + beta).max(), np.abs(JA[-1] + beta).max())
            worst_b = max(worst_b, errb / bound)
            assert errb <= bound, (kind, i, f, errb, bound)
    print(f'{env_id}: worst |J A| / terms {worst:.3g}, worst |J A_velocity + beta| / bound {worst_b:.3g}')


@pytest.mark.parametrize('env_id', MODELS)
def test_own_decision(env_id):
    """The model's own contact decision: the feet whose summed normal force
    exceeds the threshold, held at P_f = sum fn_s P_s / sum fn_s, against the
    yardstick's restatement of it from the pack (tests/ia_reference.py::own_feet,
    whose normal forces tests/test_ia_reference.py holds to the oracle's).  P_f
    within 10x the restatement's own noise, and no tighter than the project's
    1e-9 m for geometry-class outputs.  State 4 stands on two spheres of one
    foot at least, so the weights matter.  The explicit call at the reported
    feet and points repeats the result."""
    c = _case(env_id)
    ys = c.ys
    assert c.own['cactive'][0].any() and c.own['cactive'][4].any()
    assert ys.own_feet(c.q[4], c.u[4])[2].max() >= 2
    worst = 0.0
    for i in range(NS):
        fs, P, cnt, pn = ys.own_feet(c.q[i], c.u[i])
        for f in range(c.nf):
            if abs(fs[f] - OWN_THRESHOLD) > 1e-6:
                assert bool(c.own['cactive'][i, f]) == (fs[f] > OWN_THRESHOLD), (i, f, fs[f])
            if c.own['cactive'][i, f]:
                err, bound = np.abs(c.own['cpoint'][i, f] - P[f]).max(), max(10.0 * pn[f], 1e-9)
                worst = max(worst, err / bound)
                print(f'{env_id} state {i} foot {f}: {cnt[f]} spheres, fn {fs[f]:.4g} N, |P_f - yardstick| {err:.2g} m, '
                      f'bound {bound:.2g}')
                assert err <= bound, (i, f, err, bound)
            else:
                assert not c.own['cpoint'][i, f].any()
    print(f'{env_id}: worst P_f error / bound {worst:.3g}')
    again = c.ia.eval(c.q, c.u, c.ft, c.tau_act, c.ext, kind='point', cactive=c.own['cactive'],
                      cpoint=c.own['cpoint'], want=KEYS)
    assert np.array_equal(_np(again['cactive']), c.own['cactive'])
    # (not bit for bit: the point goes out and comes back through the floating origin's x)
    for k in ('accel', 'com_accel', 'reaction', 'cpoint'):
        a, b = _np(again[k]).reshape(NS, -1), c.own[k].reshape(NS, -1)
        assert (np.abs(a - b).max(1) <= 1e-9 * np.abs(b).sum(1)).all(), k


@pytest.mark.parametrize('env_id', MODELS)
def test_corners(env_id):
    c = _case(env_id)
    ia, want = c.ia, ('accel', 'com_accel', 'reaction', 'status')
    kw = dict(kind='point', cactive=c.cactive, cpoint=c.cpoint, want=want)
    same = lambda a, b: all(np.array_equal(_np(a[k]), _np(b[k])) for k in want)  # noqa: E731
    base = ia.eval(c.q, c.u, c.ft, c.tau_act, c.ext, **kw)
    assert same(base, ia.eval(c.q, c.u, c.ft, c.tau_act, c.ext, **kw))                     # a repeated call
    if c.nm:
        assert same(ia.eval(c.q, c.u, None, c.tau_act, c.ext, **kw),
                    ia.eval(c.q, c.u, np.zeros_like(c.ft), c.tau_act, c.ext, **kw))
    assert same(ia.eval(c.q, None, c.ft, c.tau_act, c.ext, **kw),
                ia.eval(c.q, np.zeros_like(c.u), c.ft, c.tau_act, c.ext, **kw))
    assert same(ia.eval(c.q, c.u, c.ft, None, None, **kw),
                ia.eval(c.q, c.u, c.ft, np.zeros_like(c.tau_act), np.zeros_like(c.ext), **kw))
    # POINT with no foot held is FORCE (its contact columns are the applied forces then)
    none = ia.eval(c.q, c.u, c.ft, c.tau_act, c.ext, kind='point', cactive=np.zeros_like(c.cactive), cpoint=c.cpoint,
                   want=want)
    for k in want:
        assert np.array_equal(_np(none[k]), c.force[k]), k
    # a state's rows do not depend on n or on its neighbours
    rep = lambda x, idx: None if x is None else x[idx]  # noqa: E731
    for n in (1, 15, 17, 33):
        idx = np.arange(n) % NS
        r = ia.eval(c.q[idx], c.u[idx], rep(c.ft, idx), c.tau_act[idx], c.ext[idx], kind='point',
                    cactive=c.cactive[idx], cpoint=c.cpoint[idx], want=want)
        for k in want:
            assert np.array_equal(_np(r[k]), _np(base[k])[idx]), (n, k)
    # a NaN in q: status -2 and zero rows, for that state only
    q = c.q.copy()
    q[3, c.nd - 1] = np.nan
    r = ia.eval(q, c.u, c.ft, c.tau_act, c.ext, **kw)
    st = _np(r['status'])
    assert st[3] == -2 and (np.delete(st, 3) == 0).all()
    for k in ('accel', 'com_accel', 'reaction'):
        v = _np(r[k])
        assert not v[3].any()
        assert np.array_equal(np.delete(v, 3, axis=0), np.delete(_np(base[k]), 3, axis=0)), k


@pytest.mark.parametrize('env_id', [W2D, TLK2D, 'TorqueWalkingImitation3D-v0'])
def test_env_path(env_id):
    """VectorEnv.induced_accelerations(kind='force') at the envs' own state."""
    import torch
    import oracle
    from bioimitation.induced_accelerations import InducedAccelerations
    from bioimitation.registry import load_pack
    from bioimitation.vector_env import VectorEnv
    pk = load_pack(env_id)
    n = 4
    rng = np.random.default_rng(5)
    envs = [VectorEnv(env_id, n, precision=64, device=0) for _ in range(2)]
    for e in envs:
        e.reset(ref_index=np.arange(n) * 7)
    for _ in range(20):
        a = torch.as_tensor(rng.uniform(0.1, 0.6, size=(n, envs[0].action_dim)), device='cuda:0')
        for e in envs:
            e.step(a)
    out = envs[0].induced_accelerations(kind='force', want=('accel', 'com_accel', 'status'))
    assert (_np(out['status']) == 0).all()
    a = torch.as_tensor(rng.uniform(0.1, 0.6, size=(n, envs[0].action_dim)), device='cuda:0')
    r0, r1 = envs[0].step(a), envs[1].step(a)
    for x, y in zip(r0[:3], r1[:3]):
        assert torch.equal(x, y)                           # the twin's next step: bit-identical
    # total = the REALIZE report's q''
    rep = _np(envs[1].osim('realize', torch.arange(n, dtype=torch.int32, device='cuda:0'), want_obs=False))
    rows = envs[1].state_rows()
    out1 = envs[1].induced_accelerations(kind='force', want=('accel',), rows=rows)
    coord_of = [cc for d in range(pk.ndof) for cc in range(pk.ncoord) if pk.coord[cc].dof == d]
    k = 2 + 2 * pk.ncoord
    qdd = rep[:, k:k + pk.ncoord][:, coord_of]
    tot = _np(out1['accel'])[:, -1]
    from bioimitation.packdef import state_row_slices
    sl, _ = state_row_slices(pk.ndof, pk.nmuscle, pk.nact, pk.horizon)
    q, u = rows[:, sl['q']], rows[:, sl['u']]
    ft = tau = None
    if pk.nmuscle:
        k = 2 + 3 * pk.ncoord + 18 * pk.nosbody + 9
        ft = rep[:, k:k + 7 * pk.nmuscle].reshape(n, pk.nmuscle, 7)[:, :, 6]
    else:
        k = 2 + 3 * pk.ncoord + 18 * pk.nosbody + 9
        tau = np.zeros((n, pk.ndof))
        for i in range(pk.ncoordact):
            if pk.coordact[i].dof >= 0:
                tau[:, pk.coordact[i].dof] += rep[:, k + i]
    # the bound: 10 x the difference the CPU yardstick shows against Oracle.forward_dynamics on the same rows
    import ia_reference as R
    ys = R.yardstick(oracle, env_id)
    rows_h = _np(rows)
    err, diff = np.zeros(n), np.zeros(n)
    for i in range(n):
        act = rows_h[i, sl['act']] if pk.nmuscle else np.zeros(1)
        lce = rows_h[i, sl['lce']] if pk.nmuscle else np.zeros(1)
        qo, mo, rc = ys.orc.forward_dynamics(_np(q)[i], _np(u)[i], act, lce, rows_h[i, sl['ctl']])
        assert rc == 0
        r = ys.eval(_np(q)[i], _np(u)[i], mo[:pk.nmuscle, 2] if pk.nmuscle else None, None if tau is None else tau[i],
                    None, kind='force')
        diff[i] = np.abs(r['accel'][-1] - qo).max()
        err[i] = np.abs(tot[i] - qdd[i]).max()
    print(f"{env_id}: |total - report q''| {err}, yardstick against forward dynamics {diff}")
    assert (err <= 10.0 * diff).all(), (err, diff)
    # the same rows through InducedAccelerations.eval: bit for bit
    ia = InducedAccelerations(env_id)
    ref = ia.eval(q, u, ft, tau, None, kind='force', want=('accel',))
    assert torch.equal(ref['accel'], out1['accel'])
    ia.close()
    for e in envs:
        e.close()
