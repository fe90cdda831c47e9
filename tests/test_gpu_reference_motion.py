"""Run-time reference motions on the GPU: refmotion.reference_from_coordinates
(its tables come from bioim_body_kin) and config['reference'] in an env.

Bounds.
  Table parity: x from the committed ref_q reproduces the committed ref_x
  within 5e-9: the committed tables went through .sto text at 10 decimals, up
  to 5e-11 per coordinate, times lever arms of about 1.5 m over up to 17
  coordinates, plus 5e-11 on the position itself: about 1.3e-9.
  Calibration: the deepest sphere penetration after penetration=0.01 is 0.01
  to 1e-12 (pelvis_ty is a pure translation: one rounding of ~1 m numbers),
  recomputed with the points and, independently, from the oracle's poses and
  the pack's sphere centres in the composite frames.
  Env against the oracle on the same pack, 10 steps from the same resets: obs,
  reward and info within 5e-9 x max(1, |value|), done equal.
Observed values are printed."""
import functools

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason='needs GPU')]

W2D, R3D, P3D = 'MuscleWalkingImitation2D-v0', 'MuscleRunningImitation3D-v0', 'MusclePalsyImitation3D-v0'
BOUND = 5e-9


def _rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def _tables(pk):
    n = pk.nrows
    return (np.array(pk.ref_time[:n]), np.ctypeslib.as_array(pk.ref_q)[:n, :pk.ncoord].copy(),
            np.ctypeslib.as_array(pk.ref_u)[:n, :pk.ncoord].copy(), np.ctypeslib.as_array(pk.ref_x)[:n].copy())


@pytest.mark.parametrize('env_id', [W2D, R3D, P3D])
def test_table_parity(env_id, tmp_path):
    from bioimitation.modelpack import pack_bytes
    from bioimitation.refmotion import reference_from_coordinates
    from bioimitation.registry import load_pack
    pk = load_pack(env_id)
    t, q, u, x = _tables(pk)
    ref = reference_from_coordinates(env_id, t, q, lowpass_hz=None, penetration=None, rebase_tx=False)
    err = np.abs(ref.x - x).max()
    print(f'{env_id}: ref_x from the committed ref_q, max difference {err:.2g} m (bound {BOUND:.2g}); '
          f'u {np.abs(ref.u - u).max():.2g}')
    free = [c for c in range(pk.ncoord) if pk.coord[c].dof >= 0]
    assert ref.x.shape == x.shape and np.array_equal(ref.q[:, free], q[:, free])
    assert np.allclose(ref.time, t, rtol=0, atol=1e-12)
    assert err <= BOUND
    # save -> {'reference': dir} is {'reference': ref} up to the storages' print precision (10 decimals)
    a = load_pack(env_id, {'reference': ref})
    b = load_pack(env_id, {'reference': ref.save(str(tmp_path / 'clip'))})
    assert (a.nrows, a.n_episode, a.reset_hi, a.cycle) == (b.nrows, b.n_episode, b.reset_hi, b.cycle)
    for x_a, x_b in zip(_tables(a), _tables(b)):
        assert np.abs(x_a - x_b).max() <= 0.5000001e-10
    for f in ('ref_time', 'ref_q', 'ref_u', 'ref_x'):
        np.ctypeslib.as_array(getattr(a, f))[...] = np.ctypeslib.as_array(getattr(b, f))
    assert pack_bytes(a) == pack_bytes(b)          # nothing but the tables differs (ref_istep included)


def test_ground_calibration():
    from bioimitation.body_kinematics import BodyKinematics
    from bioimitation.refmotion import deepest_penetration, reference_from_coordinates
    from bioimitation.registry import load_pack
    pk = load_pack(W2D)
    t, q, _, _ = _tables(pk)
    t, q = t[:120], q[:120].copy()
    q[:, pk.coord_ty] += 0.05
    q[:, pk.coord_tx] += 0.3
    ref = reference_from_coordinates(W2D, t, q, lowpass_hz=None, penetration=0.01)
    free = [c for c in range(pk.ncoord) if pk.coord[c].dof >= 0]
    qd = np.zeros((t.size, pk.ndof))
    qd[:, [pk.coord[c].dof for c in free]] = ref.q[:, free]
    bk = BodyKinematics(W2D)
    depth = deepest_penetration(bk, pk, qd)
    bk.close()
    # independently of sphere_points and the kernel: the oracle's forward kinematics, the composite frame rebuilt
    # from the first OpenSim body on it, and the pack's sphere centres in that composite frame
    import oracle
    orc = oracle.Oracle(pk)
    first = {}
    for b in range(pk.nosbody):
        first.setdefault(int(pk.osbody[b].cbody), b)
    low = np.inf
    for row in qd:
        R, p, _ = orc.fk(row)
        for s in range(pk.nsphere):
            sp = pk.sphere[s]
            ob = pk.osbody[first[int(sp.cbody)]]
            Rc = R[first[int(sp.cbody)]] @ np.array(ob.R).reshape(3, 3).T
            oc = p[first[int(sp.cbody)]] - Rc @ np.array(ob.p)
            low = min(low, (oc + Rc @ np.array(sp.loc))[1] - sp.radius)
    print(f'{W2D}: deepest penetration after calibration {depth:.15g} (asked 0.01); from the oracle\'s poses {-low:.15g}')
    assert abs(depth - 0.01) <= 1e-12
    assert abs(-low - 0.01) <= 1e-12      # heights of ~1 m numbers through two fp64 chains: a few 1e-16
    assert ref.q[0, pk.coord_tx] == 0.0 and np.allclose(np.diff(ref.q[:, pk.coord_tx]), np.diff(q[:, pk.coord_tx]), rtol=0, atol=1e-14)
    shift = ref.q[:, pk.coord_ty] - q[:, pk.coord_ty]
    assert np.ptp(shift) <= 1e-15 and abs(shift[0]) > 1e-3
    with pytest.raises(ValueError, match='a clip may be 3 to 512 rows'):
        reference_from_coordinates(W2D, np.arange(600) * 0.01, np.zeros((600, pk.ncoord)))
    with pytest.raises(ValueError, match='a clip may be 3 to 512 rows'):
        reference_from_coordinates(W2D, np.array([0.0, 0.012]), np.zeros((2, pk.ncoord)))


@functools.lru_cache(maxsize=None)
def _scaled_clip(env_id):
    """Rows 20 .. 119 of the model's own table with every joint angle scaled
    by 0.8, through reference_from_coordinates (filter, ground calibration and
    pelvis_tx rebase on)."""
    from bioimitation.obslayout import load_names
    from bioimitation.refmotion import reference_from_coordinates
    from bioimitation.registry import load_pack
    pk = load_pack(env_id)
    t, q, _, _ = _tables(pk)
    rot = np.array(load_names(env_id)['coord_rotational'], dtype=bool)
    q = q[20:120].copy()
    q[:, rot] *= 0.8
    return reference_from_coordinates(env_id, t[20:120], q)


@pytest.mark.parametrize('env_id,n', [(W2D, 8), (R3D, 4)])
def test_env_follows_the_new_tables(env_id, n):
    """The test that fails where config['reference'] is ignored."""
    import oracle
    import torch
    from bioimitation.packdef import state_row_slices
    from bioimitation.registry import load_pack
    from bioimitation.vector_env import VectorEnv
    ref = _scaled_clip(env_id)
    cfg = {'reference': ref, 'use_target_obs': True}
    pk0, pk = load_pack(env_id, {'use_target_obs': True}), load_pack(env_id, cfg)
    assert pk.nrows == 100 and pk.n_episode == 98
    assert np.abs(np.ctypeslib.as_array(pk.ref_q)[:100] - np.ctypeslib.as_array(pk0.ref_q)[20:120]).max() > 0.01
    env = VectorEnv(env_id, n, config=cfg, precision=64)
    assert env.pack.nrows == 100
    rows = np.arange(n)
    obs = env.reset(ref_index=rows).cpu().numpy()
    # q and u of row k are env k's state
    sl, _ = state_row_slices(pk.ndof, pk.nmuscle, pk.nact, pk.horizon)
    st = env.state_rows().cpu().numpy()
    free = [c for c in range(pk.ncoord) if pk.coord[c].dof >= 0]
    dofs = [pk.coord[c].dof for c in free]
    for f, tab in (('q', ref.q), ('u', ref.u)):
        assert np.array_equal(st[:, sl[f]][:, dofs], tab[:n][:, free]), f
    # the target block is row istep + 1 of the new tables
    ntrans = sum(1 for c in (pk.coord_tx, pk.coord_ty, pk.coord_tz) if c >= 0)
    k0 = 1 + (pk.ncoord - ntrans) + 2 * pk.ncoord
    notx = [c for c in range(pk.ncoord) if c != pk.coord_tx]

    def target(istep):
        r1 = np.minimum(istep + 1, pk.nrows - 1)
        return np.concatenate([ref.q[r1][:, notx], ref.u[r1][:, notx]], axis=1)
    istep = np.array([pk.ref_istep[k] for k in rows])
    assert np.array_equal(obs[:, k0:k0 + 2 * len(notx)], target(istep))
    # the oracle on the same pack, from the same resets
    orc = oracle.Oracle(pk)
    bufs = orc.new_envs(n)
    ref0 = np.stack([orc.reset(bufs, i, int(rows[i])) for i in range(n)])
    worst = dict(obs=float(_rel(obs, ref0).max()), reward=0.0, info=0.0)
    acts = np.random.default_rng(41).uniform(0, 1, size=(10, n, env.action_dim))
    for t in range(10):
        o, r, d, info = (x.cpu().numpy() for x in env.step(torch.as_tensor(acts[t], device=env.device)))
        istep = istep + 1
        assert np.array_equal(o[:, k0:k0 + 2 * len(notx)], target(istep)), t
        for i in range(n):
            oo, ro, do, io = orc.step(bufs, i, acts[t, i])
            worst['obs'] = max(worst['obs'], float(_rel(o[i], oo).max()))
            worst['reward'] = max(worst['reward'], float(_rel(r[i], ro)))
            worst['info'] = max(worst['info'], float(_rel(info[i], io).max()))
            assert bool(d[i]) == do, (t, i)
    print(f'{env_id} x{n}, 10 steps on the new tables against the oracle: worst difference / max(1, |value|) {worst}')
    assert max(worst.values()) <= BOUND, worst
    env.close()
