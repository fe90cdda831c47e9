"""The computed-muscle-control reference (tests/cmc_reference.py) against the
oracle and against itself, on the CPU: what tests/test_gpu_cmc.py compares the
kernel with is the algorithm of include/bioim.h, and its test inputs are ones
the algorithm's conditions hold on.

Bounds: the restated muscle_eval against the oracle's own, the same arithmetic
in another language: 1e-12 relative to max(1, |value|) (observed: printed);
the reachable allocation 1e-9 F0 (scipy's BVLS at tol 1e-14 on a system with
cond ~ 1e5 at lam = 1e6)."""
import numpy as np
import pytest

import cmc_reference as R

W2D, R3D, P3D = 'MuscleWalkingImitation2D-v0', 'MuscleRunningImitation3D-v0', 'MusclePalsyImitation3D-v0'
MODELS = [W2D, R3D, P3D]


@pytest.mark.parametrize('env_id', MODELS)
def test_muscle_eval_is_the_oracles(env_id):
    """Ft, vce, da/dt and dvce/dlce of the restated muscle_eval equal the
    muscle columns of Oracle.forward_dynamics at the same (q, u, act, lce, e)."""
    r = R._reference(env_id)
    rng = np.random.default_rng(5)
    worst = 0.0
    for i in range(0, R.NS, 4):
        e = rng.uniform(0, 1, size=r.pk.nact)
        _, mo, rc = r.orc.forward_dynamics(r.q[i], r.u[i], r.act[i], r.lce[i], e)
        assert rc == 0
        for m in range(r.pk.nmuscle):
            got = r.mus.eval(m, r.act[i, m], r.lce[i, m], e[m], mo[m, 0])[:4]
            ref = mo[m, [2, 3, 6, 7]]
            worst = max(worst, (np.abs(np.array(got) - ref) / np.maximum(1.0, np.abs(ref))).max())
    print(f'{env_id}: restated muscle_eval vs forward_dynamics, worst relative difference {worst:.2e}')
    assert worst <= 1e-12


@pytest.mark.parametrize('env_id', MODELS)
def test_predictor_is_monotone_in_the_excitation(env_id):
    """The end force does not decrease over e in {amin, 1/4, 1/2, 3/4, 1} on any test pair."""
    r = R._reference(env_id)
    for i in range(R.NS):
        for m in range(r.pk.nmuscle):
            es = [r.pk.muscle[m].amin, 0.25, 0.5, 0.75, 1.0]
            F = [r.mus.predict(m, r.act[i, m], r.lce[i, m], r.out['L0'][i, m], r.out['L1'][i, m], e)[0] for e in es]
            assert (np.diff(F) >= 0).all(), (env_id, i, m, F)
            assert F[0] == r.out['force_range'][i, m, 0] and F[-1] == r.out['force_range'][i, m, 1]


@pytest.mark.parametrize('env_id', MODELS)
def test_roots_are_found_and_few_pairs_are_fixed(env_id):
    """Every root solve ends within max_iter = 30 at ftol = 1e-6 (the
    condition the GPU comparison needs of its inputs); at most 10 % of the
    pairs have an empty force range; some pairs are solved, some sit on a bound."""
    r = R._reference(env_id)
    rs, fr = r.out['root_status'], r.out['force_range']
    assert (rs >= 0).all(), np.argwhere(rs < 0)
    fixed = (fr[..., 1] <= fr[..., 0]).mean()
    print(f'{env_id}: {rs.size} pairs, fixed (empty range) {100 * fixed:.1f} %, on a bound {100 * (rs == 0).mean():.1f} %, '
          f'solved {int((rs > 0).sum())} with at most {rs.max()} and on average {rs[rs > 0].mean():.1f} evaluations')
    assert fixed <= 0.10
    assert (rs > 0).sum() >= rs.size // 10 and (rs == 0).any()
    g = np.abs(r.out['predicted'] - r.out['force'])[rs > 0] / np.broadcast_to(r.f0, rs.shape)[rs > 0]
    assert (g <= R.FTOL).all()
    lo = np.array([r.mus.bracket(m)[0] for m in range(r.pk.nmuscle)])
    assert (r.out['excitation'] >= lo).all() and (r.out['excitation'] <= 1.0).all()


@pytest.mark.parametrize('env_id', MODELS)
def test_a_reachable_target_returns_its_forces(env_id):
    """tau = sum -dL/dq F for an F inside the ranges, at a large row weight
    (lam = 1e8), returns that F.  More muscles than dofs: many F give the same
    tau, and the allocation returns the one of least stress.  So F is made as
    one: x = clip(B^T mu, bounds) meets the KKT conditions of min |x|^2 subject
    to B x = tau and the box for any mu, and F = x F0.  The penalized minimizer
    x_lam obeys the same conditions with mu_lam = lam (tau - B x_lam), so
    B (x - x_lam) = mu_lam / lam with x - x_lam in the row space of the free
    columns: |x - x_lam| <= |mu| / (lam smin), smin their smallest nonzero
    singular value.  Bound: twice that (mu_lam is mu to first order) plus 1e-9
    for the BVLS solve itself (tol 1e-14 at cond ~ 1e5)."""
    r = R._reference(env_id)
    rng = np.random.default_rng(9)
    worst = 0.0
    for i in (0, 7, 20):
        L0, L1, dL = R.paths(r, r.q[i], r.u[i])
        fr = r.out['force_range'][i]
        xl, xh = fr.min(1) / r.f0, fr.max(1) / r.f0
        B = -(dL * r.f0[:, None]).T
        # of 200 random mu the one that leaves the most muscles strictly inside their (narrow) ranges
        nfree = lambda m: int(((B.T @ m > xl) & (B.T @ m < xh)).sum())  # noqa: E731
        cands = [rng.normal(0.0, 1.0, size=r.pk.ndof) * 10.0 ** rng.uniform(-5, -2) for _ in range(200)]
        mu = max(cands, key=nfree)
        x = np.clip(B.T @ mu, xl, xh)
        free = (x > xl) & (x < xh)
        assert free.sum() >= 2, (env_id, i, free.sum())
        F, tau = x * r.f0, B @ x
        s = R.solve_state(r, r.q[i], r.u[i], r.act[i], r.lce[i], tau, reserve=1e-4, roots=False)
        sv = np.linalg.svd(B[:, free], compute_uv=False)
        smin = sv[sv > 1e-9 * sv[0]].min()
        tol = 1e-9 + 2.0 * np.linalg.norm(mu) / (1e8 * smin)
        err = (np.abs(s['force'] - F) / r.f0).max()
        worst = max(worst, err)
        assert err <= tol, (env_id, i, err, tol)
        assert np.abs(s['residual']).max() <= 1e-6 * max(1.0, np.abs(tau).max())
    print(f'{env_id}: reachable targets, worst |F - F_made| / F0 = {worst:.2e}')


def test_illinois_rules_on_a_known_function():
    """The iteration of the header on g(e) = e^3 - F*: the bracket ends' values
    are reused, the count is the evaluations made, and the cap returns the
    best iterate with -1."""
    calls = []

    def P(e):
        calls.append(e)
        return (e ** 3, 0.0, 0.0)
    e, pc, st = R.illinois(P, 0.0, 1.0, 0.0, 1.0, 0.3, 1e-10)
    assert st == len(calls) > 0 and abs(e ** 3 - 0.3) <= 1e-10 and pc[0] == e ** 3 and 0.0 < e < 1.0
    del calls[:]
    e, pc, st = R.illinois(P, 0.0, 1.0, 0.0, 1.0, 0.3, 0.0, max_iter=3)
    assert st == -1 and len(calls) == 3 and e in calls
    assert abs(e ** 3 - 0.3) == min(abs(c ** 3 - 0.3) for c in calls)
