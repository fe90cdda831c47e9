"""The induced-acceleration yardstick (tests/ia_reference.py) against itself:
superposition, forward dynamics, the constraint and the momentum identity, and
the coverage and resolution of the states the GPU tests use.  CPU only."""
import functools

import numpy as np
import pytest

W2D, R3D, LK3D, TLK2D = ('MuscleWalkingImitation2D-v0', 'MuscleRunningImitation3D-v0',
                         'MuscleLockedKneeImitation3D-v0', 'TorqueLockedKneeImitation2D-v0')
MODELS = [W2D, R3D, LK3D, TLK2D]
NS = 8
NOISE_CAP = 1e-6      # of the state's largest |accel| entry


@functools.lru_cache(maxsize=None)
def _case(env_id):
    import oracle
    import ia_reference as R
    ys = R.yardstick(oracle, env_id)
    q, u, tau_act, ext, cactive, cpoint = R.draw_cases(ys, NS, seed=31)
    ft = None
    if ys.nm:
        ft = np.random.default_rng(33).uniform(10.0, 800.0, size=(NS, ys.nm))
    ev = lambda i, kind: ys.eval(q[i], u[i], None if ft is None else ft[i], tau_act[i], ext[i], kind=kind,  # noqa: E731
                                 cactive=cactive[i], cpoint=cpoint[i])
    force = [ev(i, 'force') for i in range(NS)]
    point = [ev(i, 'point') for i in range(NS)]
    return ys, q, u, ft, tau_act, ext, cactive, cpoint, force, point


@pytest.mark.parametrize('env_id', MODELS)
def test_coverage_and_noise(env_id):
    ys, q, u, ft, tau_act, ext, cactive, cpoint, force, point = _case(env_id)
    held = cactive.sum(1)
    assert (held == 0).any() and (held == 1).any() and (held == 2).any()      # flight, single and double stance
    assert np.abs(u).min() > 0
    assert np.abs(ys.orc.contact(q[0], u[0])[1]).sum() > 0                     # state 0: a Hunt-Crossley force acts
    assert ys.own_feet(q[4], u[4])[2].max() >= 2                               # state 4: a foot on two spheres
    for i in range(NS):      # the restated normal forces are the oracle's
        fs, P, cnt, pn = ys.own_feet(q[i], u[i])
        fo = ys.orc.contact(q[i], u[i])[1][1::6][:ys.nf]
        assert np.abs(fs - fo).max() <= 1e-7 * max(np.abs(fo).max(), 1.0), (i, fs, fo)
    for i in range(NS):
        assert ys.base.inside_limits(q[i], margin=1e-3)
        for r in (force[i], point[i]):
            rel = r['noise']['accel'] / np.abs(r['accel']).max()
            print(f'{env_id} state {i}: noise {r["noise"]["accel"]:.2g}, max |accel| {np.abs(r["accel"]).max():.3g}')
            assert rel <= NOISE_CAP, (i, rel)


@pytest.mark.parametrize('env_id', MODELS)
def test_identities(env_id):
    ys, q, u, ft, tau_act, ext, cactive, cpoint, force, point = _case(env_id)
    m, nf = ys.mass.sum(), ys.nf
    for i in range(NS):
        _, w = ys.orc.contact(q[i], u[i])
        for kind, r in (('force', force[i]), ('point', point[i])):
            for k in ('accel', 'com_accel', 'reaction'):
                a = r[k]
                assert np.abs(a[:-1].sum(0) - a[-1]).max() <= 1e-9 * max(np.abs(a[:-1]).sum(), 1e-300), (kind, i, k)
            # J A_c + beta = 0
            if r['J'].size:
                JA = r['accel'] @ r['J'].T
                JA[1] += r['beta']
                JA[-1] += r['beta']
                scale = np.abs(r['J']).sum() * np.abs(r['accel']).sum() + np.abs(r['beta']).sum()
                assert np.abs(JA).max() <= 1e-9 * scale, (kind, i, np.abs(JA).max(), scale)
            # m com_accel_c = sum_f reaction + [gravity] m g + [external] sum F_ext + [applied contact] F_f
            rhs = r['reaction'].sum(1)
            rhs[0] += m * ys.g
            rhs[4 + nf] += ext[i][:, :3].sum(0)
            for f in range(nf):
                if kind == 'force' or not cactive[i, f]:
                    rhs[2 + f] += w[6 * f:6 * f + 3]
            rhs[-1] = rhs[:-1].sum(0)
            lhs = m * r['com_accel']
            err = np.abs(lhs - rhs)[:, :ys.nr].max()      # a planar model's root joint carries z
            bound = 10.0 * m * max(r['noise']['com_accel'], 1e-12 * np.abs(r['com_accel']).max())
            print(f'{env_id} state {i} {kind}: momentum error {err:.2g} N, bound {bound:.2g}')
            assert err <= bound, (kind, i, err, bound)


@pytest.mark.parametrize('env_id', MODELS)
def test_force_total_is_forward_dynamics(env_id):
    """FORCE total = Oracle.forward_dynamics' q'' at matching inputs: controls
    0, and the tendon forces forward dynamics itself reports."""
    ys, q, u, *_ = _case(env_id)
    pk = ys.pk
    rng = np.random.default_rng(34)
    for i in range(NS):
        act = rng.uniform(0.05, 1.0, size=max(1, ys.nm))
        L = ys.orc.muscle_paths(q[i], u[i])[0] if ys.nm else None
        lce = np.array([ys.orc.muscle_equilibrium(m, act[m], L[m]) for m in range(ys.nm)]) if ys.nm else np.zeros(1)
        qdd, mo, rc = ys.orc.forward_dynamics(q[i], u[i], act, lce, np.zeros(max(1, pk.nact)))
        assert rc == 0
        ft = mo[:ys.nm, FT_COLUMN] if ys.nm else None
        r = ys.eval(q[i], u[i], ft, None, None, kind='force')
        err = np.abs(r['accel'][-1] - qdd).max()
        bound = 10.0 * max(r['noise']['accel'], 1e-12 * np.abs(r['accel']).max())
        print(f'{env_id} state {i}: |total - forward dynamics| {err:.2g}, bound {bound:.2g}')
        assert err <= bound, (i, err, bound)


FT_COLUMN = 2
