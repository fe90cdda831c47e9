"""The yardstick of tests/test_gpu_static_opt.py, validated on the CPU: the
BVLS reference of tests/so_reference.py satisfies the KKT conditions of the
box QP it stands for, with H and g formed independently of its least-squares
form.  Muscle IDs of test_gpu_muscle_analysis.CASES, n = 16 states each,
reserves 1 and 100 N m.

KKT of  min 1/2 a^T H a - g^T a,  lo <= a <= hi  (H = I + B^T lam B,
g = B^T lam (tau - c); the QP's objective is twice this plus a constant), with
w = g - H a:  w_m = 0 where lo < a_m < hi, w_m <= 0 at lo, w_m >= 0 at hi.
Bound: 1e-12 relative to max |A^T b| = max |g|.

The measured figures are printed (pytest -s); a prototype on this input
distribution gave: KKT residual <= 7.1e-15; cond(H) <= 9.6e4 (Walking2D),
<= 3.0e5 (3D) at reserve 1 and <= 31 at reserve 100; BVLS iterations <= 15;
about half of a state's activations at the lower bound and up to 8 at 1; no
state with l_t < 0; Palsy3D with muscles of exactly zero capacity; input
sensitivity (entries of A scaled by 1 + 1e-12 N(0, 1)) max |da| <= 9.3e-12,
the evidence behind the GPU test's 5e-9 bound on the activations.
"""
import numpy as np
import pytest

import so_reference as R

IDS = ['MuscleWalkingImitation2D-v0', 'MuscleRunningImitation3D-v0', 'MuscleLockedKneeImitation3D-v0',
       'MusclePalsyImitation3D-v0']
N = 16
KKT_TOL = 1e-12


def _kkt(H, g, a, lo, hi):
    """largest KKT violation: |w| on free variables, the wrong-signed part at the bounds"""
    w = g - H @ a
    # BVLS leaves a bound variable within rounding of its bound (seen: -8.7e-19, 3.5e-18)
    at_lo, at_hi = a <= lo + 1e-15, a >= hi - 1e-15
    free = ~(at_lo | at_hi)
    v = np.zeros_like(a)
    v[free] = np.abs(w[free])
    v[at_lo] = np.maximum(w[at_lo], 0.0)
    v[at_hi] = np.maximum(-w[at_hi], 0.0)
    return v.max()


@pytest.mark.parametrize('env_id', IDS)
def test_bvls_reference_satisfies_kkt(env_id, oracle_lib):
    r = R._reference(env_id, N)
    nd, nm = r.pk.ndof, r.pk.nmuscle
    assert r.tau.shape == (N, nd) and np.isfinite(r.tau).all()
    assert (r.Fa >= 0).all() and (r.Fp >= 0).all()
    print(env_id, 'states with l_t < 0:', int((r.lt < 0).any(1).sum()), ' zero-capacity muscles (Fa == 0):',
          int((r.Fa == 0).sum()), 'of', r.Fa.size)
    # where a dof moves a muscle's whole path the oracle's dL/dq is rounding noise around the exact 0
    # (so_reference's docstring): nothing outside the pack span is live, the noise is 1e-15, the rest is not
    assert not (r.live & ~r.span).any()
    print(env_id, 'muscles without any moment arm:', np.where(~r.live.any(1))[0].tolist())
    off = np.abs(r.dL_raw[:, ~r.live]).max()
    assert np.abs(r.dL_raw[:, r.live]).max(0).min() > 1e-3
    lam1, moved = R.row_weights(1.0, nd), 0.0
    for i in range(N):
        a0 = R.solve_state(*R.system(r.Fa[i], r.Fp[i], r.dL[i], False), r.tau[i], lam1, 0.0, 1.0)[0]
        a1 = R.solve_state(*R.system(r.Fa[i], r.Fp[i], r.dL_raw[i], False), r.tau[i], lam1, 0.0, 1.0)[0]
        moved = max(moved, np.abs(a1 - a0).max())
    print(f'{env_id} oracle |dL/dq| on rigidly moved paths <= {off:.2e} ({int((r.span & ~r.live).sum())} of '
          f'{int(r.span.sum())} span entries, {int((~r.span).sum())} outside); keeping it moves the minimizer by <= {moved:.2e}')
    assert off < 1e-14 and (r.dL[:, ~r.live] == 0.0).all() and (r.dL[:, r.live] == r.dL_raw[:, r.live]).all()
    rng = np.random.default_rng(2)
    for reserve in (1.0, 100.0):
        lam = R.row_weights(reserve, nd)
        kkt, cond, nit, n_lo, n_hi, sens = 0.0, 0.0, 0, [], [], 0.0
        for i in range(N):
            B, c = R.system(r.Fa[i], r.Fp[i], r.dL[i], False)
            a, it = R.solve_state(B, c, r.tau[i], lam, 0.0, 1.0)
            assert (a >= -1e-15).all() and (a <= 1.0 + 1e-15).all()    # BVLS's partial steps round (seen: -5.2e-18)
            H = np.eye(nm) + B.T @ (lam[:, None] * B)
            g = B.T @ (lam * (r.tau[i] - c))
            A, b = R.lsq_system(B, c, r.tau[i], lam)
            scale = np.abs(A.T @ b).max()
            assert np.allclose(A.T @ b, g, rtol=0, atol=1e-12 * max(scale, 1.0))
            k = _kkt(H, g, a, 0.0, 1.0) / max(scale, 1e-300)
            kkt, cond, nit = max(kkt, k), max(cond, np.linalg.cond(H)), max(nit, it)
            n_lo.append(int((a <= 1e-15).sum()))
            n_hi.append(int((a >= 1.0 - 1e-15).sum()))
            # the reference's input sensitivity: A's entries scaled by 1 + 1e-12 N(0, 1)
            from scipy.optimize import lsq_linear
            Ap = A * (1.0 + 1e-12 * rng.normal(size=A.shape))
            ap = lsq_linear(Ap, b, bounds=(0.0, 1.0), method='bvls', tol=1e-14).x
            sens = max(sens, np.abs(ap - a).max())
        print(f'{env_id} reserve {reserve:g}: KKT residual / max|A^T b| {kkt:.2e}  cond(H) {cond:.3g}  BVLS iterations '
              f'<= {nit}  at lo per state mean {np.mean(n_lo):.1f} of {nm}  at 1 per state max {max(n_hi)}  '
              f'sensitivity max|da| {sens:.2e}')
        assert kkt <= KKT_TOL, (reserve, kkt)


def test_formulas_follow_the_so_pin_reading(oracle_lib):
    """Fa of so_reference.capacity is SOBalance.muscle_force(fiber='rigid')
    at a = 1 without the passive force, Fa + Fp with it (tests/test_so_pin.py)"""
    import os
    from test_so_pin import SOBalance
    z = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'so_3D.npz'), allow_pickle=False))
    act = SOBalance(oracle_lib, z, fiber='rigid')
    pas = SOBalance(oracle_lib, z, fiber='rigid', passive=True)
    pk = act.pk
    rng = np.random.default_rng(3)
    from test_inverse_dynamics import _states
    q, u = _states(pk, rng, 3)
    for i in range(3):
        Fa, Fp, dL, lt = R.capacity(pk, act.orc, q[i], u[i])
        assert (lt > 0).all()          # l_t >= 0: the max(., 0) is idle and the two readings coincide
        for m in range(pk.nmuscle):
            assert act.muscle_force(q[i], u[i], m, 1.0) == pytest.approx(Fa[m], rel=1e-14, abs=1e-12)
            assert pas.muscle_force(q[i], u[i], m, 1.0) == pytest.approx(Fa[m] + Fp[m], rel=1e-13, abs=1e-12)
            assert (act._dL == dL[m]).all()
