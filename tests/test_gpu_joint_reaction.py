"""Batched joint reactions (bioim_joint_reaction, bioimitation.joint_reaction,
VectorEnv.joint_reaction) on the GPU.

States: tests/jr_reference.py::draw_states, 8 per model, strictly inside every
limited coordinate's range, u and q'' non-zero, state 0 with a foot in contact
(asserted).  Tendon forces: bioim_muscle_eval's tendon-force column at
activations U(0.05, 1).  Models: Walking2D (planar, moving points), Running3D,
LockedKnee3D (merged leg), TorqueLockedKnee2D (no muscles).

Bounds.
  Against the yardstick (tests/jr_reference.py, independent Newton-Euler from
  differentiated poses): reaction and tau_joint within 10x the yardstick's own
  h-vs-h/2 noise of that state and output; point and muscle_wrench, which the
  yardstick forms without differences (noise 0), within the project's bound
  for geometry-class outputs, 1e-9 x (1 m, resp. the state's sum |Ft|).
  Observed (fp64): noise 3e-7 .. 3e-6 N at sum |W_k| = 1e3 .. 8e4 N; the
  kernel's error against the yardstick is of the noise's own size (the
  yardstick's), see DESIGN.md 5.17.
  Exact identities (fp64): 1e-9 x the state's sum of |force terms|
  (sum_k |W_k| + sum_m |Ft_m| + |ext|).
  fp32: 10x the error that the fp32-rounded inputs cause in the fp64 kernel.
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
KEYS = ('reaction', 'point', 'tau_joint', 'muscle_wrench')
RESIDUAL = 4


def _np(t):
    return t.double().cpu().numpy()


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(env_id):
    """The model's solver objects, test states, tendon forces and yardstick
    values (computed once, shared, read-only)."""
    import oracle
    import jr_reference as J
    from bioimitation.inverse_dynamics import InverseDynamics
    from bioimitation.joint_reaction import JointReaction
    from bioimitation.muscle_analysis import MuscleAnalysis
    c = Case()
    c.ys = J.yardstick(oracle, env_id)
    c.jr = JointReaction(env_id)
    c.id = InverseDynamics(env_id)
    c.q, c.u, c.a = J.draw_states(c.ys, NS, seed=21)
    c.nm = c.ys.nm
    c.ft = c.dldq = None
    if c.nm:
        ma = MuscleAnalysis(env_id)
        act = np.random.default_rng(22).uniform(0.05, 1.0, size=(NS, c.nm))
        r = ma.eval(c.q, c.u, act=act, want=('fiber', 'dldq'))
        c.ft, c.dldq = _np(r['fiber'])[:, :, 2].copy(), _np(r['dldq'])
        ma.close()
    c.ref = [c.ys.eval(c.q[i], c.u[i], c.a[i], None if c.ft is None else c.ft[i]) for i in range(NS)]
    c.out = {k: _np(v) for k, v in c.jr.eval(c.q, c.u, c.a, c.ft, frame='ground', want=KEYS).items()}
    c.terms = np.array([r['scale'] for r in c.ref]) + (np.abs(c.ft).sum(1) if c.nm else 0.0)
    for a in vars(c).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def _about_origin(reaction, point):
    """[.., nb, 6] about c_b -> about the ground origin"""
    r = reaction.copy()
    r[..., 3:] += np.cross(point, reaction[..., :3])
    return r


@pytest.mark.parametrize('env_id', MODELS)
def test_against_yardstick(env_id):
    c = _case(env_id)
    ys = c.ys
    assert np.abs(ys.orc.contact(c.q[0], c.u[0])[1]).sum() > 0          # state 0: a foot in contact
    assert np.abs(c.u).min() > 0 and np.abs(c.a).min() > 0
    worst = {k: 0.0 for k in KEYS}
    for i in range(NS):
        r = c.ref[i]
        ftsum = np.abs(c.ft[i]).sum() if c.nm else 0.0
        bounds = dict(reaction=10.0 * r['noise']['reaction'], tau_joint=10.0 * r['noise']['tau_joint'],
                      point=1e-9, muscle_wrench=1e-9 * ftsum)
        for k in KEYS:
            err = np.abs(c.out[k][i] - r[k]).max()
            worst[k] = max(worst[k], err / r['scale'] if k != 'point' else err)
            print(f'{env_id} state {i} {k}: sum|W| {r["scale"]:.3g} noise {r["noise"][k]:.2g} err {err:.2g} '
                  f'bound {bounds[k]:.2g}')
            assert err <= bounds[k], (i, k, err, bounds[k])
    print(f'{env_id}: worst error / sum|W| (point: m): {worst}')
    if env_id == W2D:
        # the planar model's out-of-plane loads: non-zero in the yardstick, and covered by the comparison above
        for i in range(NS):
            for b in (1, 4):
                assert np.abs(c.ref[i]['reaction'][b, [2, 3, 4]]).min() > 1e-3
        assert np.abs(c.out['reaction'][:, [1, 4]][:, :, [2, 3, 4]]).min() > 1e-3
    if env_id == TLK2D:
        assert not c.out['muscle_wrench'].any()


@pytest.mark.parametrize('env_id', MODELS)
def test_exact_identities(env_id):
    c = _case(env_id)
    ys, nd = c.ys, c.ys.nd
    res = _np(c.id.eval(RESIDUAL, c.q, c.u, c.a))
    rhs = res.copy()
    mdof = ys.moving_dofs()
    if c.nm:
        rhs += np.einsum('imd,im->id', c.dldq, c.ft)
        for i in range(NS):
            rhs[i] -= c.ref[i]['mob']        # non-zero only on the moving points' own dofs
            assert not np.delete(c.ref[i]['mob'], mdof).any()
        if env_id == W2D:
            assert mdof and max(np.abs(c.ref[i]['mob']).max() for i in range(NS)) > 0.1
    tol = 1e-9 * c.terms
    e_tau = np.abs(c.out['tau_joint'] - rhs)
    plain = [d for d in range(nd) if d not in mdof]
    print(f'{env_id}: tau_joint identity: {e_tau[:, plain].max():.2g} (moving-point dofs '
          f'{e_tau[:, mdof].max() if mdof else 0:.2g}), bound {tol.min():.2g}')
    assert (e_tau <= tol[:, None]).all()
    # the muscles' forces are internal
    e_mw = np.abs(c.out['muscle_wrench'].sum(1)).max(1)
    print(f'{env_id}: sum_k muscle_wrench: {e_mw.max():.2g}')
    assert (e_mw <= tol).all()
    # root reaction = the sum of every body's own wrench W_k, at the identities' bound, two ways.
    # (a) W_k taken back out of the call's own rows, W_k = F_k - sum of k's children's F (each moved from its
    #     c_b to the ground origin with `point`): the subtree sums and the shifts to c_b, no yardstick in it.
    F0 = _about_origin(c.out['reaction'], c.out['point'])
    par = np.array(ys.parent)
    Wk = F0.copy()
    for k in range(ys.nb):
        if par[k] >= 0:
            Wk[:, par[k]] -= F0[:, k]
    e_a = np.abs(F0[:, 0] - Wk.sum(1)).max(1)
    assert (e_a <= tol).all()
    # (b) W_k is no output, so the independent W_k are the yardstick's.  Where the yardstick resolves the bound
    #     (NB x its noise on W within it) the bound is asserted as it stands; on the other states (light
    #     TorqueLockedKnee2D ones, where 1e-9 of the terms is below the yardstick's 1e-6 N) the sum can be no
    #     better than its NB noisy terms, and 10 x NB x noise is the bound.
    e_b, seen = np.zeros(NS), np.zeros(NS, bool)
    for i in range(NS):
        e_b[i] = np.abs(F0[i, 0] - c.ref[i]['W'].sum(0)).max()
        seen[i] = ys.nb * c.ref[i]['noise']['W'] <= tol[i]
        assert e_b[i] <= (tol[i] if seen[i] else 10.0 * ys.nb * c.ref[i]['noise']['W']), (i, e_b[i], tol[i])
    print(f'{env_id}: root reaction = sum W_k: from the call\'s own rows {e_a.max():.2g}; against the yardstick\'s W_k '
          f'{e_b[seen].max() if seen.any() else 0:.2g} on {int(seen.sum())} resolved states (bound {tol[seen].min() if seen.any() else 0:.2g}), '
          f'{e_b[~seen].max() if (~seen).any() else 0:.2g} on the {int((~seen).sum())} others')
    if env_id != TLK2D:
        assert seen.any()
    # frames: CHILD / PARENT rotate back onto GROUND
    R = np.stack([r['R'] for r in c.ref])                      # [n][nb][3][3], body -> ground
    for frame, Rf in (('child', R), ('parent', np.where((par >= 0)[None, :, None, None], R[:, par], np.eye(3)))):
        o = _np(c.jr.eval(c.q, c.u, c.a, c.ft, frame=frame)['reaction'])
        back = np.concatenate([np.einsum('nbij,nbj->nbi', Rf, o[..., :3]), np.einsum('nbij,nbj->nbi', Rf, o[..., 3:])], -1)
        e = np.abs(back - c.out['reaction']).reshape(NS, -1).max(1)
        print(f'{env_id}: {frame} frame rotated back: {e.max():.2g}')
        assert (e <= tol).all()
        if frame == 'child':
            assert np.abs(o - c.out['reaction']).max() > 1.0      # it did rotate
    neg = _np(c.jr.eval(c.q, c.u, c.a, c.ft, frame='ground', on='parent')['reaction'])
    assert np.array_equal(neg, -c.out['reaction'])
    # ext: a wrench on the right foot moves the right leg's chain and the root by exactly that wrench
    foot = 3
    chain = [b for b in range(ys.nb) if ys.sub[b, foot]]
    other = [b for b in range(ys.nb) if b not in chain]
    assert chain == [0, 1, 2, 3] and other
    ext = np.zeros((NS, ys.nb, 6))
    ext[:, foot] = np.random.default_rng(23).uniform(-300, 300, size=(NS, 6))
    o = {k: _np(v) for k, v in c.jr.eval(c.q, c.u, c.a, c.ft, ext=ext, frame='ground', want=KEYS).items()}
    d = _about_origin(o['reaction'], o['point']) - _about_origin(c.out['reaction'], c.out['point'])
    e = np.abs(d[:, chain] + ext[:, [foot]]).reshape(NS, -1).max(1)
    print(f'{env_id}: ext on the foot: {e.max():.2g}')
    assert (e <= tol + 1e-9 * np.abs(ext).reshape(NS, -1).sum(1)).all()
    assert np.array_equal(o['reaction'][:, other], c.out['reaction'][:, other])
    assert np.array_equal(o['muscle_wrench'], c.out['muscle_wrench']) and np.array_equal(o['point'], c.out['point'])


@pytest.mark.parametrize('env_id', [W2D, R3D, LK3D, TLK2D])
def test_corners(env_id):
    import torch
    c = _case(env_id)
    jr = c.jr
    full = jr.eval(c.q, c.u, c.a, c.ft, want=KEYS)
    if c.nm:      # ft = 0 equals ft = NULL bit for bit
        a, b = jr.eval(c.q, c.u, c.a, None, want=KEYS), jr.eval(c.q, c.u, c.a, np.zeros_like(c.ft), want=KEYS)
        for k in KEYS:
            assert torch.equal(a[k], b[k]), k
        assert not a['muscle_wrench'].any()
    z = np.zeros_like(c.q)
    a, b = jr.eval(c.q, None, None, c.ft, want=KEYS), jr.eval(c.q, z, z, c.ft, want=KEYS)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    a, b = jr.eval(c.q, c.u, c.a, c.ft, contact=False), jr.eval(c.q, c.u, c.a, c.ft, contact=True)
    assert not torch.equal(a['reaction'][0], b['reaction'][0])           # state 0 stands on a foot
    # a state's rows do not depend on n or on the other states, and a repeated call repeats them
    for n in (1, 15, 17, 33):
        idx = np.arange(n) % NS
        idx[0] = 5
        args = [x[idx] if x is not None else None for x in (c.q, c.u, c.a, c.ft)]
        o1, o2 = jr.eval(*args, want=KEYS), jr.eval(*args, want=KEYS)
        for k in KEYS:
            assert torch.equal(o1[k], o2[k]), (n, k)
            assert torch.equal(o1[k], full[k][torch.as_tensor(idx, device=full[k].device)]), (n, k)
    assert jr.eval(c.q[:0], want=KEYS)['reaction'].shape == (0, c.ys.nb, 6)


@pytest.mark.parametrize('env_id', [W2D, R3D, TLK2D])
def test_fp32_against_fp64(env_id):
    """The fp32 kernel against the fp64 result; the measure is the error that
    the fp32-rounded inputs (q, u, q'', ft) cause in the fp64 kernel, the bound
    10x that, each the maximum over the 8 states per output.

    An fp32 handle's call converts at its loads and stores and computes in
    fp64 on an fp64 image of the model (include/bioim.h says why: contact
    stiffness times the error of an fp32 kinematic chain), so what is left is
    the rounding of the inputs and of the outputs, and this test is about the
    conversions.  Observed, fp32 / measure: reaction Walking2D 2.82e-3 / 2.66e-3 N
    (1.06x), Running3D 1.40e-3 / 1.39e-3, TorqueLockedKnee2D 3.18e-3 / 3.22e-3;
    point at most 8.1e-8 / 5.5e-8 m; muscle_wrench at most 1.0e-3 / 6.0e-4 N."""
    from bioimitation.joint_reaction import JointReaction
    c = _case(env_id)
    r32 = lambda x: None if x is None else x.astype(np.float32).astype(np.float64)   # noqa: E731
    args = (c.q, c.u, c.a, c.ft)
    rounded = {k: _np(v) for k, v in c.jr.eval(*map(r32, args), frame='ground', want=KEYS).items()}
    j32 = JointReaction(env_id, precision=32)
    got = {k: _np(v) for k, v in j32.eval(*args, frame='ground', want=KEYS).items()}
    j32.close()
    over = []
    for k in KEYS:
        e_in = np.abs(rounded[k] - c.out[k]).max()
        e32 = np.abs(got[k] - c.out[k]).max()
        print(f'{env_id} {k}: fp32-rounded inputs through fp64 {e_in:.3g}, fp32 kernel {e32:.3g}')
        if not e32 <= 10.0 * e_in:
            over.append((k, e32, e_in))
    assert not over, over


@pytest.mark.parametrize('env_id', [W2D, R3D])
def test_env_joint_reaction(env_id, tmp_path):
    """VectorEnv.joint_reaction on 4 envs after 20 steps: a read (a twin env's
    next step is bit-identical), equal to JointReaction.eval fed the same
    report rows, and on a muscle env the ground-pelvis reaction and the
    floating dofs' tau_joint vanish (a free body's root joint carries nothing)
    within 10x what the yardstick gives when fed Oracle.forward_dynamics' own
    q'' at the same state.  The planar model's root joint is free in the plane
    only: fx, fy, mz vanish, while fz, mx, my are the loads that keep the model
    in its plane (about 20 N / N m here, in the yardstick as on the GPU), so
    on Walking2D the in-plane components are the ones checked; Running3D's
    root is free in all six."""
    import torch
    from bioimitation.packdef import state_row_slices
    from bioimitation.simulation_io import split_osim_report
    from bioimitation.vector_env import VectorEnv
    c = _case(env_id)
    ys, n = c.ys, 4
    free_comp = [0, 1, 5] if env_id == W2D else [0, 1, 2, 3, 4, 5]
    a, b = (VectorEnv(env_id, n, precision=64, seed=3) for _ in range(2))
    pk = a.pack
    rng = np.random.default_rng(24)
    acts = torch.as_tensor(rng.uniform(0, 1, size=(21, n, a.action_dim)), device=a.device)
    for e in (a, b):
        e.reset(ref_index=[4, 20, 36, 52])
        for t in range(20):
            e.step(acts[t])
    got = a.joint_reaction(frame='ground', want=KEYS)
    assert not getattr(a, '_realize_sync', False)          # the realize that reads nothing back
    assert got.table.joints == c.jr.joints and (got.frame, got.on) == ('ground', 'child')
    part = a.joint_reaction(env_ids=[2, 0], frame='ground', want=('reaction', 'tau_joint'))
    for k in part:
        assert torch.equal(part[k], got[k][[2, 0]]), k
    # the env's result labels itself for write_sto
    from bioimitation import joint_reaction as jrmod, storage
    jrmod.write_sto(str(tmp_path / 'env.sto'), 0.01 * np.arange(n), a.joint_reaction(want=('reaction', 'point')))
    labels = storage.read_sto(str(tmp_path / 'env.sto'))[1]
    assert labels[10] == 'hip_r_on_femur_r_in_femur_r_fx' and len(labels) == 1 + 9 * pk.ncbody
    rows, rep = a.state_rows(), a.osim_report.clone()
    ra, rb = a.step(acts[20]), b.step(acts[20])
    for x, y, what in zip(ra, rb, ('obs', 'reward', 'done', 'info')):
        assert torch.equal(x, y), what
    # the same rows through JointReaction.eval
    sl, _ = state_row_slices(pk.ndof, pk.nmuscle, pk.nact, pk.horizon)
    s, rp = _np(rows), _np(rep)
    q, u, act, lce = (s[:, sl[f]] for f in ('q', 'u', 'act', 'lce'))
    free = [cc for cc in range(pk.ncoord) if pk.coord[cc].dof >= 0]
    dofs = [pk.coord[cc].dof for cc in free]
    qdd, ft = np.zeros((n, pk.ndof)), np.zeros((n, pk.nmuscle))
    for i in range(n):
        sp = split_osim_report(pk, rp[i])
        qdd[i, dofs] = sp['qdd'][free]
        ft[i] = sp['muscles'][:, 6]
    want = c.jr.eval(q, u, qdd, ft, frame='ground', want=KEYS)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    # a free body's root joint carries nothing
    root_dofs = sorted(pk.coord[cc].dof for cc in range(pk.ncoord) if pk.coord[cc].cbody == 0 and pk.coord[cc].dof >= 0)
    g = {k: _np(v) for k, v in got.items()}
    for i in range(n):
        qdd_o, mo, rc = ys.orc.forward_dynamics(q[i], u[i], act[i], lce[i], act[i])
        assert rc == 0
        y = ys.eval(q[i], u[i], qdd_o, mo[:pk.nmuscle, 2])
        floor_r, floor_t = np.abs(y['reaction'][0, free_comp]).max(), np.abs(y['tau_joint'][root_dofs]).max()
        e_r, e_t = np.abs(g['reaction'][i, 0, free_comp]).max(), np.abs(g['tau_joint'][i, root_dofs]).max()
        if env_id == W2D:     # the planar root joint's own load: the same on both sides
            assert np.abs(g['reaction'][i, 0] - y['reaction'][0]).max() <= 10.0 * y['noise']['reaction'] + 1e-9 * y['scale']
        print(f'{env_id} env {i}: root reaction {e_r:.3g} (yardstick on the oracle\'s q\'\' {floor_r:.3g}), floating tau_joint '
              f'{e_t:.3g} ({floor_t:.3g}); hip_r load {np.abs(g["reaction"][i, 1, :3]).max():.4g} N')
        assert e_r <= 10.0 * floor_r and e_t <= 10.0 * floor_t
        assert np.abs(g['reaction'][i, 1:, :3]).max() > 10.0      # while the leg joints do carry load
    a.close()
    b.close()
