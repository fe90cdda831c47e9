"""ReflexDrive (bioimitation.reflex): the stretch-reflex tracking drive of
tests/tracking.py on the device, MuscleWalkingImitation2D-v0 in fp64.

Open loop it gives the CPU TrackingDrive's excitations on the same states;
closed loop, with no host data in the loop, it keeps the ROWS_UP envs up for
200 steps and lets the ROWS_FALL ones fall exactly as the oracle run under the
CPU drive does (tests/test_tracking_drive.py establishes that outcome)."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason='needs GPU')]

ENV_ID = 'MuscleWalkingImitation2D-v0'


def _rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def test_reflex_drive_tracks_like_the_cpu_drive():
    """First 5 steps: the device excitations equal the CPU drive's on
    get_state() rows to 1e-9 absolute.  All 200 steps are driven by
    ReflexDrive alone; the oracle envs run beside them under the CPU drive
    on their own state.  `done` agrees at every step, every ROWS_UP env is
    alive at step 200 and the four ROWS_FALL envs have fallen, and obs and
    reward stay within the bound of test_parity_200_steps_c3_tracking_drive
    on the envs alive on both sides: 1e-4, and max(1e-7, 100 x the error of
    the oracle's one-ulp twin)."""
    import oracle
    import torch
    from tracking import ROWS_FALL, ROWS_UP, TrackingDrive
    from bioimitation.obslayout import load_names
    from bioimitation.reflex import GAINS, ReflexDrive
    from bioimitation.registry import load_pack
    from bioimitation.vector_env import VectorEnv
    import tracking
    assert GAINS == tracking.GAINS                 # the same default gains
    rows = ROWS_UP + ROWS_FALL[:4]
    n, T = len(rows), 200
    pk = load_pack(ENV_ID)
    env = VectorEnv(ENV_ID, n, precision=64, auto_reset=False)
    orc = oracle.Oracle(pk)
    cpu = TrackingDrive(orc, pk, load_names(ENV_ID))
    bufs, twin = orc.new_envs(n), orc.new_envs(n)
    env.reset(ref_index=rows)
    for i, r in enumerate(rows):
        orc.reset(bufs, i, r)
        orc.reset(twin, i, r)
        s = orc.get_state(twin, i)
        s[5] = np.nextafter(s[5], np.inf)          # one ulp in the first coordinate
        orc.set_state(twin, i, s)
    drive = ReflexDrive(env)
    # the reference tables are the oracle's
    assert np.abs(drive.Lref.cpu().numpy() - cpu.Lref).max() < 1e-9
    assert np.abs(drive.Ldref.cpu().numpy() - cpu.Ldref).max() < 1e-9
    live = np.ones(n, bool)                        # alive on the GPU, the oracle and the twin
    orc_alive, gpu_alive = np.ones(n, bool), np.ones(n, bool)
    e_gpu, e_twin, e_open = np.zeros(T), np.zeros(T), 0.0
    for t in range(T):
        ex = drive()
        assert ex.shape == (n, pk.nmuscle) and ex.dtype == env.dtype and ex.device == env.device
        if t < 5:
            s = env.get_state()
            want = np.stack([cpu(s[i]) for i in range(n)])
            e_open = max(e_open, np.abs(ex.cpu().numpy() - want).max())
            assert e_open < 1e-9, (t, e_open)
        obs, rew, done = (v.cpu().numpy() for v in env.step(ex)[:3])
        for i in range(n):
            a = cpu(orc.get_state(bufs, i))
            o, r, d, _ = orc.step(bufs, i, a)
            o2, r2, d2, _ = orc.step(twin, i, a)
            if live[i]:
                e_gpu[t] = max(e_gpu[t], _rel(obs[i], o).max(), abs(rew[i] - r) / max(1.0, abs(r)))
                e_twin[t] = max(e_twin[t], _rel(o2, o).max(), abs(r2 - r) / max(1.0, abs(r)))
                assert bool(done[i]) == d, (t, i)
            orc_alive[i] &= not d
            gpu_alive[i] &= not bool(done[i])
            live[i] = live[i] and not (d or d2 or done[i])
    ks = [0, 49, 99, 149, 199]
    print(f'{ENV_ID} 200 steps under ReflexDrive: open-loop excitation err {e_open:.1e}; alive at t=200 oracle '
          f'{orc_alive.sum()}/{n}, GPU {gpu_alive.sum()}/{n}; max rel err GPU vs oracle / oracle vs its one-ulp twin at t=' +
          ', '.join(f'{k + 1}: {e_gpu[k]:.1e} / {e_twin[k]:.1e}' for k in ks) + f'; overall {e_gpu.max():.1e}')
    nu = len(ROWS_UP)
    assert gpu_alive[:nu].all() and not gpu_alive[nu:].any(), gpu_alive
    assert orc_alive[:nu].all() and not orc_alive[nu:].any(), orc_alive
    assert e_gpu.max() < 1e-4, (int(e_gpu.argmax()), e_gpu.max())
    assert (e_gpu <= np.maximum(1e-7, 100 * e_twin)).all(), int(np.argmax(e_gpu / np.maximum(1e-30, e_twin)))
    env.close()


def test_reflex_drive_offset_moves_the_joint_targets():
    """the optional per-env joint offset, (N, <= 8), as the CPU drive's"""
    import oracle
    import torch
    from tracking import TrackingDrive
    from bioimitation.obslayout import load_names
    from bioimitation.reflex import ReflexDrive
    from bioimitation.registry import load_pack
    from bioimitation.vector_env import VectorEnv
    pk = load_pack(ENV_ID)
    n = 6
    env = VectorEnv(ENV_ID, n, precision=64)
    env.reset(ref_index=[1, 5, 17, 24, 46, 51])
    rng = np.random.default_rng(3)
    env.step(torch.as_tensor(rng.uniform(0, 1, size=(n, env.action_dim)), device=env.device))
    cpu = TrackingDrive(oracle.Oracle(pk), pk, load_names(ENV_ID))
    drive = ReflexDrive(env, gains=dict(kl=15.0))
    cpu15 = TrackingDrive(cpu.orc, pk, load_names(ENV_ID), dict(kl=15.0))
    s = env.get_state()
    for width in (8, 6, 2):
        off = rng.normal(0, 0.05, size=(n, width))
        got = drive(torch.as_tensor(off)).cpu().numpy()
        want = np.stack([cpu15(s[i], off[i]) for i in range(n)])
        assert np.abs(got - want).max() < 1e-9, width
        assert np.abs(got - np.stack([cpu15(s[i]) for i in range(n)])).max() > 1e-3   # and it matters
    with pytest.raises(ValueError, match='offset must have shape'):
        drive(torch.zeros((n, 9)))
    with pytest.raises(ValueError, match='offset must have shape'):
        drive(torch.zeros((n + 1, 8)))
    env.close()


def test_reflex_drive_refuses_a_torque_env():
    from bioimitation.reflex import ReflexDrive
    from bioimitation.vector_env import VectorEnv
    env = VectorEnv('TorqueWalkingImitation2D-v0', 2)
    with pytest.raises(ValueError, match='torque env'):
        ReflexDrive(env)
    env.close()
