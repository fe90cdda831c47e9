"""Per-env external body forces of the batched step (bioim_set_external_forces,
VectorEnv.set_external_forces) on the GPU.  fp64 unless said otherwise.

1. Oracle parity, free-running: the protocol, bound (1e-6, `done` equal) and
   print of test_perturbation_parity_fp64.  The device holds a step's forces
   over all its substeps and its closing realize; the oracle's force is a table
   of time, and a step's closing realize and the next step's first substep lie
   at the same time.  So the oracle env gets step k's force as a one-entry
   table (one value at all times) before each of its steps: the same hold.
   (A table that switches a quarter substep before each step boundary gives the
   closing realize the NEXT step's force, which the device cannot know.)
2. General wrenches at acceleration level against the numpy yardstick
   (tests/ia_reference.py), the form and bound of
   test_gpu_induced_accel.py::test_env_path plus 1e-9 x the summed magnitudes of
   the yardstick's external column; `ext` built from Oracle.fk frames.
3. A body-frame point against the same point given in ground: the suite's
   realize bound (TOL_REALIZE of test_gpu_frontend.py).
4. Independence of the envs, and a NaN force.
5. Removal and the realize cache (the bound of test_gpu_realize_cache.py).
6. rollout() == step() x T, unfused.
7. fp32: the new path against the push table.
8. A mixed batch with forces on one segment launches unfused.
Observed values are printed."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason='needs a HIP GPU')]

T2D, M2D = 'TorqueWalkingImitation2D-v0', 'MuscleWalkingImitation2D-v0'
R3D, LK3D, T3D = 'MuscleRunningImitation3D-v0', 'MuscleLockedKneeImitation3D-v0', 'TorqueWalkingImitation3D-v0'
TOL_REALIZE = 5e-9      # tests/test_gpu_frontend.py
CACHE_BOUND = 5e-9      # tests/test_gpu_realize_cache.py:32


def _np(t):
    return t.double().cpu().numpy() if t.is_floating_point() else t.cpu().numpy()


def _rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def _bodies(env_id):
    from bioimitation.obslayout import load_names
    return list(load_names(env_id)['bodies'])


def _welded(pk, bodies):
    """an OpenSim body that is not the first of its composite body (it is
    welded into another body's), the last such one that is neither the torso nor calcn_r"""
    first = {}
    for b in range(pk.nosbody):
        first.setdefault(pk.osbody[b].cbody, b)
    cand = [b for b in range(pk.nosbody) if first[pk.osbody[b].cbody] != b and bodies[b] not in ('torso', 'calcn_r')]
    assert cand, 'no welded OpenSim body'
    return bodies[cand[-1]]


def _actions(env_id, rng, n, a_dim, pk, rows, scale=1.0):
    """tests/test_gpu_parity.py::_actions"""
    if 'Muscle' in env_id:
        return scale * rng.uniform(0.0, 1.0, size=(n, a_dim))
    base = np.array([[pk.ref_q[min(r, pk.nrows - 1)][pk.pd_coord[i]] for i in range(a_dim)] for r in rows])
    return base + rng.normal(0.0, 0.05, size=(n, a_dim))


def _env(env_id, n, precision=64, **kw):
    from bioimitation.vector_env import VectorEnv
    return VectorEnv(env_id, n, precision=precision, seed=3, **kw)


def _t(env, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=env.device, dtype=env.dtype)


def _step(env, a):
    """a step's outputs, copied (the env reuses its buffers)"""
    return tuple(x.clone() for x in env.step(a))


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize('env_id', [T2D, M2D, R3D, LK3D])
def test_oracle_parity_fp64(env_id):
    import oracle
    import torch
    from bioimitation.registry import load_pack
    rng = np.random.default_rng(9)
    n, T = 32, 30
    pk, bodies = load_pack(env_id), _bodies(env_id)
    slots = ['torso', 'calcn_r', _welded(pk, bodies)]
    ob = [bodies.index(b) for b in slots]
    assert pk.osbody[ob[2]].cbody in [pk.osbody[b].cbody for b in range(ob[2])]
    rows = rng.integers(0, 120, size=n)
    env = _env(env_id, n)
    orc = oracle.Oracle(pk)
    bufs = orc.new_envs(n)
    w = env.set_external_forces(slots)           # zeros; body-frame points at the origins
    assert w.shape == (n, 3, 9) and not w.any()
    env.reset(ref_index=rows)
    for i in range(n):
        orc.reset(bufs, i, int(rows[i]))
    alive = np.ones(n, bool)
    worst, pushed = 0.0, 0
    host = np.zeros((n, 3, 9))
    for t in range(T):
        st = np.array([orc.get_state(bufs, i)[1] for i in range(n)]).astype(int)
        acts = _actions(env_id, rng, n, env.action_dim, pk, st + 1, scale=0.4)
        f = rng.choice([-50.0, 0.0, 50.0], size=n)
        host[:] = 0.0
        host[np.arange(n), np.arange(n) % 3, 0] = f
        w.copy_(_t(env, host))                   # between steps, on the env's stream
        obs, rew, done, info = env.step(_t(env, acts))
        obs, rew, done, info = (_np(v) for v in (obs, rew, done, info))
        for i in range(n):
            if not alive[i]:
                continue
            orc.set_perturbation(bufs, i, ob[i % 3], [0.0], [f[i]])
            o, r, d, inf = orc.step(bufs, i, acts[i])
            e = max(_rel(obs[i], o).max(), abs(rew[i] - r), _rel(info[i], inf).max())
            assert e < 1e-6, (t, i, slots[i % 3], e)
            assert bool(done[i]) == d, (t, i)
            worst = max(worst, e)
            pushed += f[i] != 0
            alive[i] = alive[i] and not d
    print(f'{env_id} external forces on {slots} fp64 {T} steps: max rel err {worst:.2e}, alive {alive.sum()}/{n}, '
          f'{pushed} pushed env-steps')
    assert pushed > n
    # the forces are live: without them the step differs
    env.reset(ref_index=rows)
    a = _t(env, _actions(env_id, rng, n, env.action_dim, pk, rows + 1, scale=0.4))
    host[:] = 0.0
    host[np.arange(n), np.arange(n) % 3, 0] = 50.0
    w.copy_(_t(env, host))
    o_push = _step(env, a)[0]
    w.zero_()
    env.reset(ref_index=rows)
    o_free = _step(env, a)[0]
    assert (o_push != o_free).any(dim=1).all()
    env.close()


# ------------------------------------------------------------------ 2
def _report_parts(pk, rep, n):
    """q'' (dof order), tendon forces and actuator torques per dof of REALIZE report rows"""
    coord_of = [cc for d in range(pk.ndof) for cc in range(pk.ncoord) if pk.coord[cc].dof == d]
    k = 2 + 2 * pk.ncoord
    qdd = rep[:, k:k + pk.ncoord][:, coord_of]
    k = 2 + 3 * pk.ncoord + 18 * pk.nosbody + 9
    ft = tau = None
    if pk.nmuscle:
        ft = rep[:, k:k + 7 * pk.nmuscle].reshape(n, pk.nmuscle, 7)[:, :, 6]
    else:
        tau = np.zeros((n, pk.ndof))
        for i in range(pk.ncoordact):
            if pk.coordact[i].dof >= 0:
                tau[:, pk.coordact[i].dof] += rep[:, k + i]
    return qdd, ft, tau


@pytest.mark.parametrize('env_id', [M2D, T2D, T3D])
def test_general_wrench_acceleration(env_id):
    import oracle
    import torch
    import ia_reference as R
    from bioimitation.packdef import state_row_slices
    from bioimitation.registry import load_pack
    pk, bodies = load_pack(env_id), _bodies(env_id)
    n = 4
    rng = np.random.default_rng(5)
    env = _env(env_id, n)
    env.reset(ref_index=np.arange(n) * 7)
    for _ in range(20):
        env.step(_t(env, rng.uniform(0.1, 0.6, size=(n, env.action_dim))))
    slots = ['torso', 'calcn_r', 'calcn_r', _welded(pk, bodies)]       # two on one body
    planar = pk.coord_tz < 0

    def vec(most, comps):
        """random directions (within `comps`), lengths in [0.2, 1] x most"""
        v = np.zeros((n, 4, 3))
        v[:, :, comps] = rng.normal(size=(n, 4, len(comps)))
        return v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.uniform(0.2, 1.0, size=(n, 4, 1)) * most
    # |F| <= 100 N, off-origin body-frame points |p| <= 0.2 m, |T| <= 20 N m; a planar model: force and point in
    # the plane, torque about z
    host = np.concatenate([vec(100.0, [0, 1] if planar else [0, 1, 2]), vec(0.2, [0, 1] if planar else [0, 1, 2]),
                           vec(20.0, [2] if planar else [0, 1, 2])], axis=2)
    ids = torch.arange(n, dtype=torch.int32, device=env.device)
    rows = env.state_rows()
    sl, _ = state_row_slices(pk.ndof, pk.nmuscle, pk.nact, pk.horizon)
    rows_h = _np(rows)
    q, u = rows_h[:, sl['q']], rows_h[:, sl['u']]
    qdd0, ft, tau = _report_parts(pk, _np(env.osim('realize', ids, want_obs=False)), n)
    w = env.set_external_forces(slots, _t(env, host))
    qdd, ft1, tau1 = _report_parts(pk, _np(env.osim('realize', ids, want_obs=False)), n)
    tot = _np(env.induced_accelerations(kind='force', want=('accel',), rows=rows)['accel'])[:, -1]
    assert (np.abs(qdd - qdd0).max(1) > 1e-2).all()                      # the forces act
    if ft is not None:
        assert np.array_equal(ft, ft1)                                   # tendon forces do not depend on them
    ys = R.yardstick(oracle, env_id)
    ob = [bodies.index(b) for b in slots]
    for i in range(n):
        Rb, pb, _ = ys.orc.fk(q[i])
        ext = np.zeros((pk.ncbody, 6))
        for j, b in enumerate(ob):
            F, p, Tq = host[i, j, 0:3], host[i, j, 3:6], host[i, j, 6:9]
            P = pb[b] + Rb[b] @ p
            ext[pk.osbody[b].cbody, :3] += F
            ext[pk.osbody[b].cbody, 3:] += np.cross(P, F) + Tq
        act = rows_h[i, sl['act']] if pk.nmuscle else np.zeros(1)
        lce = rows_h[i, sl['lce']] if pk.nmuscle else np.zeros(1)
        qo, mo, rc = ys.orc.forward_dynamics(q[i], u[i], act, lce, rows_h[i, sl['ctl']])
        assert rc == 0
        fti = mo[:pk.nmuscle, 2] if pk.nmuscle else None
        taui = None if tau is None else tau[i]
        r0 = ys.eval(q[i], u[i], fti, taui, None, kind='force')
        r1 = ys.eval(q[i], u[i], fti, taui, ext, kind='force')
        diff = np.abs(r0['accel'][-1] - qo).max()
        terms = np.abs(r1['accel'][4 + ys.nf]).sum()
        bound = 10.0 * diff + 1e-9 * terms
        err = np.abs(qdd[i] - r1['accel'][-1]).max()
        err_ia = np.abs(tot[i] - r1['accel'][-1]).max()
        print(f"{env_id} env {i}: |realize q'' - yardstick| {err:.3g}, |induced total - yardstick| {err_ia:.3g}, "
              f"bound {bound:.3g} (yardstick against forward dynamics {diff:.3g}, external column {terms:.3g})")
        assert err <= bound, (i, err, bound)
        assert err_ia <= bound, (i, err_ia, bound)
    # the analyses' ext is the device's own: the same wrench from body_kinematics frames
    xg = _np(env.external_wrench_ground())
    assert xg.shape == (n, pk.ncbody, 6) and np.abs(xg).max() > 1.0
    env.close()


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize('env_id', [M2D, R3D])
def test_point_frames(env_id):
    import torch
    from bioimitation.registry import load_pack
    pk, bodies = load_pack(env_id), _bodies(env_id)
    n = 4
    rng = np.random.default_rng(7)
    env = _env(env_id, n)
    env.reset(ref_index=60 + 9 * np.arange(n))
    for _ in range(20):
        env.step(_t(env, 0.4 * rng.uniform(0.0, 1.0, size=(n, env.action_dim))))
    body = _welded(pk, bodies)
    b = bodies.index(body)
    ids = torch.arange(n, dtype=torch.int32, device=env.device)
    host = rng.uniform(-1.0, 1.0, size=(n, 1, 9)) * np.array([80.0] * 3 + [0.15] * 3 + [15.0] * 3)
    if pk.coord_tz < 0:
        host[:, :, [2, 5, 6, 7]] = 0.0
    coord_of = [cc for d in range(pk.ndof) for cc in range(pk.ncoord) if pk.coord[cc].dof == d]
    k = 2 + 2 * pk.ncoord

    def qdd():
        return _np(env.osim('realize', ids, want_obs=False))[:, k:k + pk.ncoord][:, coord_of]
    env.set_external_forces([body], _t(env, host), point_in='body')
    a_body = qdd()
    bk = env.body_kinematics(want=('origin', 'rot'))
    o, Rm = _np(bk['origin'])[:, b, 0, :], _np(bk['rot'])[:, b, :].reshape(n, 3, 3)
    assert (np.abs(o[:, 0]) > 0.5).all(), o[:, 0]       # pelvis x (the floating origin) far from 0
    ground = host.copy()
    ground[:, 0, 3:6] = o + np.einsum('nij,nj->ni', Rm, host[:, 0, 3:6])
    env.set_external_forces([body], _t(env, ground), point_in='ground')
    a_ground = qdd()
    env.set_external_forces(None)
    a_none = qdd()
    err = np.abs(a_body - a_ground).max(1)
    bound = TOL_REALIZE * np.maximum(1.0, np.abs(a_body).max(1))
    print(f"{env_id} {body}: body-frame against ground-frame point, |q'' difference| {err}, bound {bound}, "
          f"forces move q'' by {np.abs(a_body - a_none).max(1)}")
    assert (err <= bound).all(), (err, bound)
    assert (np.abs(a_body - a_none).max(1) > 1e-2).all()
    env.close()


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize('env_id', [M2D, T3D])
def test_independence_and_nan(env_id):
    import torch
    from bioimitation.registry import load_pack
    pk = load_pack(env_id)
    n, j = 20, 17                       # two workgroups; env j in the second
    rng = np.random.default_rng(8)
    rows = rng.integers(0, 100, size=n)
    host = rng.uniform(-30.0, 30.0, size=(n, 2, 9)) * np.array([1.0] * 3 + [0.005] * 3 + [0.3] * 3)
    a, b = _env(env_id, n), _env(env_id, n)
    wa = a.set_external_forces(['torso', 'calcn_l'], _t(a, host))
    other = host.copy()
    other[j] = -2.0 * host[j]
    wb = b.set_external_forces(['torso', 'calcn_l'], _t(b, other))
    for e in (a, b):
        e.reset(ref_index=rows)
    keep = np.arange(n) != j
    acts = [_t(a, _actions(env_id, rng, n, a.action_dim, pk, rows + 1 + t, scale=0.4)) for t in range(6)]
    moved = False
    for t in range(5):
        ra, rb = _step(a, acts[t]), _step(b, acts[t])
        for x, y in zip(ra, rb):
            assert torch.equal(x[keep], y[keep]), t
        moved = moved or not torch.equal(ra[0][j], rb[0][j])
    assert moved
    # a NaN force on env j: done there at that step, every other env as before
    wb.copy_(wa)
    b.load_state(a.state_rows())
    wb[j, 1, 1] = float('nan')
    ra, rb = _step(a, acts[5]), _step(b, acts[5])
    assert int(rb[2][j]) == 1
    for x, y in zip(ra, rb):
        assert torch.equal(x[keep], y[keep])
    assert torch.isfinite(rb[0][keep]).all()
    for e in (a, b):
        e.close()


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize('env_id', [M2D, T2D, R3D, T3D])
def test_removal_and_realize_cache(env_id):
    import torch
    from bioimitation.registry import load_pack
    pk = load_pack(env_id)
    n = 20
    rng = np.random.default_rng(10)
    rows = rng.integers(0, 100, size=n)
    a, b = _env(env_id, n), _env(env_id, n)
    for e in (a, b):
        e.reset(ref_index=rows)
    acts = [_t(a, _actions(env_id, rng, n, a.action_dim, pk, rows + 1 + t, scale=0.4)) for t in range(8)]
    a.step(acts[0])                               # a default step: the realize cache is live
    b.load_state(a.state_rows())
    w = a.set_external_forces(['torso', 'calcn_r'],
                              _t(a, rng.uniform(-40.0, 40.0, size=(n, 2, 9)) * np.array([1.0] * 3 + [0.05] * 3 + [0.2] * 3)))
    for t in range(1, 4):
        a.step(acts[t])
    assert a.set_external_forces(None) is None and a.external_forces is None
    b.load_state(a.state_rows())
    worst = 0.0
    for t in range(4, 7):
        ra, rb = _step(a, acts[t]), _step(b, acts[t])
        if pk.nmuscle:
            e = max(_rel(_np(ra[0]), _np(rb[0])).max(), np.abs(_np(ra[1]) - _np(rb[1])).max())
            worst = max(worst, e)
            assert e <= CACHE_BOUND, (t, e)
            assert torch.equal(ra[2], rb[2])
        else:
            for x, y in zip(ra, rb):
                assert torch.equal(x, y), t
    # zero-valued forces against none, one step
    b.load_state(a.state_rows())
    a.set_external_forces(['torso', 'calcn_r'])
    ra, rb = _step(a, acts[7]), _step(b, acts[7])
    e0 = max(_rel(_np(ra[0]), _np(rb[0])).max(), np.abs(_np(ra[1]) - _np(rb[1])).max())
    print(f'{env_id}: after removal, 3 steps against a twin without forces: max rel diff {worst:.2e}; '
          f'zero forces against none: {e0:.2e} (bound {CACHE_BOUND:.0e})')
    assert e0 <= CACHE_BOUND, e0
    assert torch.equal(ra[2], rb[2])
    assert w.shape == (n, 2, 9)
    for e in (a, b):
        e.close()


# ------------------------------------------------------------------ 6
@pytest.mark.parametrize('env_id', [M2D, T3D])
def test_rollout_equals_steps(env_id):
    import torch
    from bioimitation.registry import load_pack
    pk = load_pack(env_id)
    n, T = 20, 4
    rng = np.random.default_rng(11)
    rows = rng.integers(0, 100, size=n)
    host = rng.uniform(-40.0, 40.0, size=(n, 2, 9)) * np.array([1.0] * 3 + [0.05] * 3 + [0.2] * 3)
    a, b = _env(env_id, n), _env(env_id, n)
    for e in (a, b):
        e.set_external_forces(['torso', 'calcn_r'], _t(e, host), point_in=['body', 'ground'])
        e.reset(ref_index=rows)
    plan = torch.stack([_t(a, _actions(env_id, rng, n, a.action_dim, pk, rows + 1 + t, scale=0.4)) for t in range(T)])
    obs, rew, done, info = a.rollout(plan, obs='all', info=True)
    assert a.last_rollout_fused is False
    for t in range(T):
        o, r, d, i = _step(b, plan[t])
        assert torch.equal(obs[t], o) and torch.equal(rew[t], r) and torch.equal(done[t], d) and torch.equal(info[t], i), t
    assert torch.equal(a.state_rows(), b.state_rows())
    # without forces the same plan runs fused and differs
    a.set_external_forces(None)
    a.reset(ref_index=rows)
    obs0 = a.rollout(plan, obs='all')[0]
    assert a.last_rollout_fused is True
    assert not torch.equal(obs0, obs)
    for e in (a, b):
        e.close()


# ------------------------------------------------------------------ 7
FP32_OBSERVED = 4.705e-2  # observed max over the 10 steps (MI355X), of max(1, |value|): the test asserts 10 x this


def test_fp32_against_the_push_table():
    """A constant 50 N ground-x force at the torso origin through the new path
    against the push table (the reference here) on fp32 handles, 10 steps,
    n = 8.  The two differ in three lines of arithmetic (the moment's sums);
    free-running fp32 trajectories then part ways through the contact
    transitions (tests/test_gpu_parity.py: fp32 resolves q'' to 0.2 of
    max(|q''|, 1)), so the difference is that of two fp32 runs, not of the
    forces: observed 4.705e-2 over the 10 steps (the first step alone is
    printed), bound 10 x that."""
    import torch
    from bioimitation.registry import load_pack
    env_id = M2D
    pk = load_pack(env_id)
    n, T = 8, 10
    rng = np.random.default_rng(12)
    rows = rng.integers(0, 100, size=n)
    a, b = _env(env_id, n, precision=32), _env(env_id, n, precision=32)
    host = np.zeros((n, 1, 9))
    host[:, 0, 0] = 50.0
    a.set_external_forces(['torso'], _t(a, host))
    b.set_perturbation(np.array([0.0, 100.0]), np.full((n, 2), 50.0))
    for e in (a, b):
        e.reset(ref_index=rows)
    worst, first = 0.0, None
    for t in range(T):
        act = _t(a, 0.4 * rng.uniform(0.0, 1.0, size=(n, a.action_dim)))
        ra, rb = _step(a, act), _step(b, act)
        worst = max(worst, _rel(_np(ra[0]), _np(rb[0])).max(), np.abs(_np(ra[1]) - _np(rb[1])).max())
        first = worst if first is None else first
        assert torch.equal(ra[2], rb[2]), t
    bound = 10.0 * FP32_OBSERVED
    print(f'{env_id} fp32, external force against the push table, {T} steps: max rel diff {worst:.3e} '
          f'(first step {first:.3e}; bound {bound:.3e})')
    assert worst <= bound, (worst, bound)
    for e in (a, b):
        e.close()


# ------------------------------------------------------------------ 8
def test_mixed_batch_launches_unfused():
    """Forces on one segment of the fused pair (LockedKnee3D + Palsy3D): the
    group step and the group rollout run one launch per segment; the other
    segment's rows stay what the fused launch gives, bit for bit."""
    import torch
    from bioimitation.vector_env import MixedVectorEnv
    segs = [(LK3D, 3), ('MusclePalsyImitation3D-v0', 2)]
    a, b = (MixedVectorEnv(segs, precision=64, seed=5) for _ in range(2))
    rng = np.random.default_rng(13)
    rows = rng.integers(0, 100, size=5)
    for m in (a, b):
        m.reset(ref_index=rows)
    w = a.set_external_forces(1, ['torso', 'calcn_r'])
    assert w.shape == (2, 2, 9) and a.envs[1].external_forces is not None and a.envs[0].external_forces is None
    act = torch.as_tensor(0.4 * rng.uniform(0.0, 1.0, size=(5, a.action_dim)), device=a.device)
    ra, rb = (tuple(x.clone() for x in m.step(act)) for m in (a, b))
    assert a.last_step_fused is False and b.last_step_fused is True
    assert torch.equal(ra[0][:3], rb[0][:3]) and torch.equal(ra[1][:3], rb[1][:3])
    e0 = _rel(_np(ra[0][3:]), _np(rb[0][3:])).max()               # zero-valued forces against none
    assert e0 <= CACHE_BOUND, e0
    w[:, 0, 0] = 60.0
    ra, rb = (tuple(x.clone() for x in m.step(act)) for m in (a, b))
    assert torch.equal(ra[0][:3], rb[0][:3])
    assert (ra[0][3:] != rb[0][3:]).any(dim=1).all()
    plan = torch.stack([act, act])
    a.rollout(plan)
    b.rollout(plan)
    assert a.last_rollout_fused is False and b.last_rollout_fused is True
    print(f'mixed batch, forces on segment 1: unfused; zero forces against none {e0:.2e} (bound {CACHE_BOUND:.0e})')
    for m in (a, b):
        m.close()
