"""The CPU yardstick of tests/ik_reference.py, checked on its own: it is what
tests/test_gpu_inverse_kinematics.py compares bioim_ik_solve with, on the same
frames (every 6th frame of each shipped IK trial) and the same synthetic
problems.  No GPU.

Recorded here (printed by the tests; DESIGN.md 5.16 lists them):
- iterations, 3D trial: warm 7-12, cold 9-17; 02905 trial, warm: 19-152;
- frames that do not finish at the cap (200 / 400): none (UNFINISHED is empty);
- cond(J^T W J) of the synthetic problems: see COND_MAX (no model's marker
  subset is rank-deficient, so no case needs coordinate tasks).
"""
import numpy as np
import pytest

import ik_reference as R

TRIALS = ['3D', '02905']
BOUNDS = {'3D': (5e-3, 2e-2), '02905': (5e-3, 2e-2)}     # test_ik_pin.BOUNDS: median / max distance to OpenSim's q
UNFINISHED = {('3D', 'warm'): [], ('3D', 'cold'): [], ('02905', 'warm'): []}   # frame indices that hit the cap
# The yardstick's own Gauss-Newton step at its solutions: a step-size stop at
# tol on a linearly converging iteration (rate rho) leaves rho / (1 - rho) tol
# to the minimizer, <= 20 tol for rho <= 0.95 (the 02905 trial: rho ~ 0.9).
# Observed: 1.4e-10 (3D), 1.4e-9 (02905).
FLOOR_MAX = 20 * R.TOL
# rank deficiency would show as cond ~ 1 / eps; observed <= 1.7e3 on every model
COND_MAX = 1e6


@pytest.mark.parametrize('tag,start', list(UNFINISHED))
def test_yardstick_finishes(tag, start, oracle_lib):
    sol = R.trial_solution(oracle_lib, tag, start)
    st = sol['status']
    done = st[st >= 0]
    print(f'{tag} {start}: {len(st)} frames, iterations {done.min()}-{done.max()}, '
          f'unfinished {list(sol["frames"][st < 0])}')
    assert len(UNFINISHED[(tag, start)]) <= 0.05 * len(st)
    assert list(sol['frames'][st < 0]) == UNFINISHED[(tag, start)]
    assert (done >= 1).all()


def test_cold_start_reaches_the_warm_solution(oracle_lib):
    warm, cold = R.trial_solution(oracle_lib, '3D', 'warm'), R.trial_solution(oracle_lib, '3D', 'cold')
    d = np.abs(warm['q'] - cold['q']).max()
    print(f'3D: cold vs warm {d:.2e}')
    assert d < 1e-8


@pytest.mark.parametrize('tag', TRIALS)
def test_solution_is_near_opensims(tag, oracle_lib):
    z, mm = R.trial_model(oracle_lib, tag)
    sol = R.trial_solution(oracle_lib, tag, 'warm')
    dist = np.abs(sol['q'] - sol['q0']).max(axis=1)      # the warm start is OpenSim's q
    print(f'{tag}: distance to OpenSim median {np.median(dist):.2e}, max {dist.max():.2e}')
    assert np.median(dist) < BOUNDS[tag][0] and dist.max() < BOUNDS[tag][1]


@pytest.mark.parametrize('tag', TRIALS)
def test_solution_is_stationary(tag, oracle_lib):
    floor = R.noise_floor(oracle_lib, tag)
    print(f'{tag}: largest Gauss-Newton step at the yardstick\'s solutions {floor:.2e}')
    assert floor < FLOOR_MAX


@pytest.mark.parametrize('env_id', R.SYNTHETIC)
def test_synthetic_recovery(env_id, oracle_lib):
    mm, w, qstar = R.synthetic_model(oracle_lib, env_id)
    qs = qstar[::8]
    q0 = R.synthetic_start(mm, qs, 1)
    worst, its, conds = 0.0, [], []
    for k in range(len(qs)):
        x = mm.markers(qs[k])
        _, A, _ = R.normal_equations(mm, qs[k], x, w)
        conds.append(np.linalg.cond(A))
        q, s = R.solve(mm, x, w, q0[k], tol=1e-10, max_iter=50)
        assert 1 <= s <= 50
        its.append(s)
        worst = max(worst, np.abs(q - qs[k]).max())
    print(f'{env_id}: {mm.nm} markers, recovery {worst:.2e}, iterations {min(its)}-{max(its)}, '
          f'cond(J^T W J) <= {max(conds):.2e}')
    assert worst <= 1e-8
    assert max(conds) < COND_MAX


def test_chain_mask_matches_the_jacobian(oracle_lib):
    """The root-chain table the GPU test uses for the exact zeros: a dof off a
    marker's chain does not move it."""
    z, mm = R.trial_model(oracle_lib, '3D')
    J = mm.jacobian(mm.qdof(z['q'][10]))
    on = mm.chain_mask()
    assert (J[~on[:, None, :].repeat(3, 1)] == 0).all()
    assert (np.abs(J).max(axis=1)[on] > 0).mean() > 0.9
