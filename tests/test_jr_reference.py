"""The CPU yardstick of bioim_joint_reaction (tests/jr_reference.py) against the
exact projection identity on the oracle: per dof d,

    S_d . F_cb(d)  =  RESIDUAL_d + lim_d                       (Oracle.id_eval)
                      + sum_m dL_m/dq_d Ft_m                   (Oracle.muscle_paths)
                      - sum_m Ft_m (g . dP/dq_d)_m             (moving points)

The first muscle term takes the muscles' generalized force back out of the
balance (tau_mus = -sum_m dL_m/dq_d Ft_m), the second leaves in what is not a
body force: a moving point's own-coordinate term is a mobility force
(-Ft g . dP/dq on its coordinate), which the coordinate itself carries, so it
stays in S_d . F with that sign.  The states lie strictly inside every limited
coordinate's range, so every lim_d is exactly 0 (asserted from the pack's limit
table).  The yardstick differentiates poses numerically; its bound here is 10x
its own h-vs-h/2 noise plus 1e-9 of the state's force terms (the columns S_d
are central differences too, and their error is not in the time-step noise).
Observed: noise 2e-7 .. 3e-6 N at sum |W_k| of 1e3 .. 4e4 N, identity error
below the noise on every state."""
import numpy as np
import pytest

import oracle
import jr_reference as J

MODELS = ['MuscleWalkingImitation2D-v0', 'MuscleRunningImitation3D-v0', 'MuscleLockedKneeImitation3D-v0',
          'TorqueLockedKneeImitation2D-v0']
RESIDUAL = 4   # include/bioim.h BIOIM_ID_RESIDUAL


@pytest.mark.parametrize('env_id', MODELS)
def test_projection_identity_and_muscle_balance(env_id):
    ys = J.yardstick(oracle, env_id)
    n = 4
    Q, U, A = J.draw_states(ys, n, seed=11)
    rng = np.random.default_rng(12)
    # every limit force is exactly 0: the states are inside [qlow, qup] of every limited dof
    assert ys.limits or env_id.startswith('Torque')
    for i in range(n):
        for d, lo, up in ys.limits:
            assert lo < Q[i, d] < up
    assert np.abs(ys.orc.contact(Q[0], U[0])[1]).sum() > 0    # a foot in contact
    for i in range(n):
        ft = rng.uniform(0.0, 1500.0, ys.nm) if ys.nm else None
        r = ys.eval(Q[i], U[i], A[i], ft)
        rhs = ys.orc.id_eval(RESIDUAL, Q[i], U[i], A[i])
        terms = np.abs(r['W']).sum()
        if ys.nm:
            _, _, dldq = ys.orc.muscle_paths(Q[i], U[i])
            rhs = rhs + dldq.T @ ft - r['mob']
            terms += np.abs(ft).sum()
            if env_id == 'MuscleWalkingImitation2D-v0':
                assert np.abs(r['mob']).max() > 0.1    # the model has moving points and they carry load
            # the muscles' forces are internal: their wrenches sum to zero over the bodies
            assert np.abs(r['muscle_wrench'].sum(0)).max() <= 1e-12 * np.abs(ft).sum()
            assert np.abs(r['muscle_wrench']).max() > 1.0
        err = np.abs(r['tau_joint'] - rhs).max()
        bound = 10.0 * r['noise']['tau_joint'] + 1e-9 * terms
        print(f'{env_id} state {i}: sum|W| {r["scale"]:.3g}  noise {r["noise"]["tau_joint"]:.2g}  err {err:.2g}  '
              f'bound {bound:.2g}')
        assert r['noise']['tau_joint'] < 1e-8 * terms      # the yardstick resolves 1e-8 of the terms
        assert err <= bound
        # the root's reaction is the sum of every body's own wrench
        np.testing.assert_allclose(r['reaction'][0, :3], r['W'][:, :3].sum(0), rtol=0, atol=1e-9 * terms)


def test_planar_model_has_out_of_plane_loads():
    """Walking2D's hips sit off the plane: the yardstick's mx, my and the
    lateral force of the muscles on the hip rows are not zero."""
    ys = J.yardstick(oracle, 'MuscleWalkingImitation2D-v0')
    Q, U, A = J.draw_states(ys, 1, seed=11)
    ft = np.full(ys.nm, 500.0)
    r = ys.eval(Q[0], U[0], A[0], ft)
    for b in (1, 4):     # hip_r, hip_l
        assert np.abs(r['reaction'][b, [2, 3, 4]]).min() > 1e-2, r['reaction'][b]
    r0 = ys.eval(Q[0], U[0], A[0], None)     # without muscles: moments only
    for b in (1, 4):
        assert np.abs(r0['reaction'][b, [3, 4]]).min() > 1e-3 and abs(r0['reaction'][b, 2]) < 1e-6
