"""Batched muscle analysis (bioim_muscle_eval, bioimitation.muscle_analysis,
VectorEnv.muscle_analysis) against the fp64 oracle.

States as tests/test_inverse_dynamics.py::_states (reference rows + N(0, 0.02)
on q, N(0, 0.2) on u, default_rng(1)), activations U(0.01, 1).  IDs: Muscle
Walking2D with n = 200 (13 workgroups, a partial last one) and Running3D,
LockedKnee3D, Palsy3D with n = 64: every muscle topology class (planar,
spatial, locked-knee spatial) and the palsy parameters.  The oracle reference
of an ID is computed once and shared.

Bounds (metric: max |out - ref| / max(1, row max |ref|), a row = one state's
values of the quantity): geometry the id_kernel test's own, 1e-9 fp64 /
2e-3 fp32; fiber columns 5e-9 fp64 / 2e-3 fp32; tau 1e-9 relative to
max(1, max |ref|).  Observed maxima are printed (DESIGN.md 5.14 lists them).
"""
import functools

import numpy as np
import pytest

from conftest import gpu_available
from test_inverse_dynamics import _states

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason='needs GPU')]

CASES = [('MuscleWalkingImitation2D-v0', 200), ('MuscleRunningImitation3D-v0', 64),
         ('MuscleLockedKneeImitation3D-v0', 64), ('MusclePalsyImitation3D-v0', 64)]
GEOM_TOL = {64: 1e-9, 32: 2e-3}
FIBER_TOL = {64: 5e-9, 32: 2e-3}
TAU_TOL = 1e-9


class Ref:
    pass


@functools.lru_cache(maxsize=None)
def _reference(env_id, n):
    """The oracle's values on the test states (read-only, shared)."""
    import oracle
    from bioimitation.registry import load_pack
    pk = load_pack(env_id)
    orc = oracle.Oracle(pk)
    rng = np.random.default_rng(1)
    nm, nd = pk.nmuscle, pk.ndof
    r = Ref()
    r.pk, r.orc = pk, orc
    r.q, r.u = _states(pk, rng, n)
    r.act = rng.uniform(0.01, 1.0, size=(n, nm))
    r.L, r.Ld, r.dL = np.zeros((n, nm)), np.zeros((n, nm)), np.zeros((n, nm, nd))
    for i in range(n):
        r.L[i], r.Ld[i], r.dL[i] = orc.muscle_paths(r.q[i], r.u[i])
    r.lmin = np.array([pk.muscle[m].lmin for m in range(nm)])
    r.lopt = np.array([pk.muscle[m].lopt for m in range(nm)])
    r.lce_eq = np.array([[orc.muscle_equilibrium(m, r.act[i, m], r.L[i, m]) for m in range(nm)] for i in range(n)])
    r.lce_given = np.maximum(r.lce_eq * (1.0 + rng.normal(0.0, 0.02, size=(n, nm))), r.lmin)

    def fd(u, lce):
        mo = np.zeros((n, nm, 8))
        for i in range(n):
            _, mo[i], rc = orc.forward_dynamics(r.q[i], u[i], r.act[i], lce[i], r.act[i])
            assert rc == 0, (env_id, i)          # no state may drop out
        return mo
    r.mo_eq, r.mo_given = fd(r.u, r.lce_eq), fd(r.u, r.lce_given)
    r.mo_eq_u0 = fd(np.zeros_like(r.u), r.lce_eq)
    for a in vars(r).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


def _rel(out, ref):
    """max |out - ref| / max(1, row max |ref|), rows = states"""
    out, ref = out.reshape(len(ref), -1), ref.reshape(len(ref), -1)
    return (np.abs(out - ref) / np.maximum(1.0, np.abs(ref).max(1, keepdims=True))).max()


def _fiber_ref(lce, mo):
    """[n][nm][5] in FIBER_COLUMNS order from the fiber lengths and the
    oracle's muscle_out (L, Ldot, Ft, vce, Ff, Fa, dadt, dvdl)"""
    return np.stack([lce, mo[:, :, 3], mo[:, :, 2], mo[:, :, 4], mo[:, :, 5]], axis=2)


def _pack_span(pk):
    """[nm][nd] bool: the dofs on the root paths of a muscle's path-point
    bodies, without the dofs that move every body (the floating base)"""
    nd = pk.ndof
    own = [set() for _ in range(pk.ncbody)]
    for c in range(pk.ncoord):
        if pk.coord[c].dof >= 0:
            own[pk.coord[c].cbody].add(pk.coord[c].dof)

    def path(b):
        s = set()
        while b >= 0:
            s |= own[b]
            b = pk.cbody[b].parent
        return s
    root = set.intersection(*[path(b) for b in range(pk.ncbody)])
    span = np.zeros((pk.nmuscle, nd), bool)
    for m in range(pk.nmuscle):
        mu = pk.muscle[m]
        for j in range(mu.npt):
            span[m, sorted(path(pk.pathpt[mu.pt_off + j].cbody) - root)] = True
    return span


def _np(t):
    return t.double().cpu().numpy()


@pytest.mark.parametrize('env_id,n', CASES)
def test_geometry_matches_oracle(env_id, n):
    """length, speed, dldq against orc.muscle_paths; dldq exactly 0 outside
    each muscle's pack span (the floating-base dofs among them)"""
    from bioimitation.muscle_analysis import MuscleAnalysis
    r = _reference(env_id, n)
    span = _pack_span(r.pk)
    assert span.any(1).all() and not span.all(1).any()
    for precision in (64, 32):
        ma = MuscleAnalysis(env_id, precision=precision)
        assert len(ma.muscle_names) == r.pk.nmuscle and len(ma.coordinate_names) == r.pk.ncoord
        out = ma.eval(r.q, r.u, want=('length', 'speed', 'dldq', 'moment_arms'))
        assert all(v.dtype == ma.dtype and v.device == ma.device for v in out.values())
        L, Ld, dL = _np(out['length']), _np(out['speed']), _np(out['dldq'])
        assert (_np(out['moment_arms']) == -dL).all()
        errs = dict(length=_rel(L, r.L), speed=_rel(Ld, r.Ld), dldq=_rel(dL, r.dL))
        print(env_id, precision, 'geometry max rel err', {k: f'{v:.2e}' for k, v in errs.items()})
        for k, e in errs.items():
            assert e < GEOM_TOL[precision], (k, precision, e)
        assert (dL[:, ~span] == 0.0).all()
        # without u the speed is 0, and single outputs come alone
        only = ma.eval(r.q, want=('speed',))
        assert set(only) == {'speed'} and (_np(only['speed']) == 0.0).all()
        ma.close()


@pytest.mark.parametrize('env_id,n', CASES)
def test_fiber_and_tau_match_oracle(env_id, n):
    """fiber columns against the oracle's forward dynamics at the same
    (q, u, act, lce), with given fiber lengths and with lce=None (the oracle's
    static equilibrium per muscle first); tau against -dLdq^T Ft of the
    oracle's values"""
    from bioimitation.muscle_analysis import MuscleAnalysis
    r = _reference(env_id, n)
    at_lmin = int((r.lce_eq <= r.lmin).sum())
    print(env_id, 'equilibrium fibers at lmin:', at_lmin, 'of', r.lce_eq.size)
    for precision in (64, 32):
        ma = MuscleAnalysis(env_id, precision=precision)
        for name, lce_in, lce_ref, mo in (('given', r.lce_given, r.lce_given, r.mo_given), ('equilibrium', None, r.lce_eq, r.mo_eq)):
            out = ma.eval(r.q, r.u, r.act, lce_in, want=('fiber', 'tau'))
            fib, tau = _np(out['fiber']), _np(out['tau'])
            ref = _fiber_ref(lce_ref, mo)
            errs = [_rel(fib[:, :, c], ref[:, :, c]) for c in range(5)]
            tau_ref = -np.einsum('imd,im->id', r.dL, mo[:, :, 2])
            e_tau = np.abs(tau - tau_ref).max() / max(1.0, np.abs(tau_ref).max())
            print(env_id, precision, name, 'fiber max rel err (length, velocity, Ft, Ff, Fa)',
                  ' '.join(f'{e:.2e}' for e in errs), 'tau', f'{e_tau:.2e}')
            for c, e in enumerate(errs):
                assert e < FIBER_TOL[precision], (name, precision, c, e)
            assert e_tau < (TAU_TOL if precision == 64 else 2e-3), (name, precision, e_tau)
        ma.close()


@pytest.mark.parametrize('env_id,n', CASES)
def test_equilibrium_is_static(env_id, n):
    """lce=None at u = 0: the fiber velocity vanishes (|v| / l_opt < 1e-9)
    for the fibers above lmin, as in the oracle (<= 9.3e-11 there on these states)"""
    from bioimitation.muscle_analysis import MuscleAnalysis
    r = _reference(env_id, n)
    ma = MuscleAnalysis(env_id, precision=64)
    fib = _np(ma.eval(r.q, None, r.act, None, want=('fiber',))['fiber'])
    ma.close()
    free = fib[:, :, 0] > r.lmin
    assert free.sum() > 0.9 * free.size
    v = np.abs(fib[:, :, 1]) / r.lopt
    vo = np.abs(r.mo_eq_u0[:, :, 3]) / r.lopt
    print(env_id, 'static equilibrium: max |v| / l_opt', f'{v[free].max():.2e}', 'oracle', f'{vo[r.lce_eq > r.lmin].max():.2e}',
          'fibers at lmin', int((~free).sum()))
    assert v[free].max() < 1e-9
    assert _rel(fib[:, :, 0], r.lce_eq) < FIBER_TOL[64]


def _report_fiber(env, ids):
    """FIBER_COLUMNS of the listed envs from the bioim_osim REALIZE report"""
    pk = env.pack
    rep = _np(env.osim('realize', ids, want_obs=False))[ids]
    o = 2 + 3 * pk.ncoord + 18 * pk.nosbody + 9
    m = rep[:, o:o + 7 * pk.nmuscle].reshape(len(ids), pk.nmuscle, 7)
    # activation, fiber_length, fiber_velocity, fiber_force, active_fiber_force, excitation, tendon_force
    return np.stack([m[:, :, 1], m[:, :, 2], m[:, :, 6], m[:, :, 3], m[:, :, 4]], axis=2)


def test_env_muscle_analysis_reads_the_envs():
    """VectorEnv.muscle_analysis at the envs' state: bit for bit
    MuscleAnalysis.eval on get_state()'s q, u, act, lce; the fiber columns
    are the REALIZE report's (warm-started roots there, cold here)"""
    import torch
    from bioimitation.muscle_analysis import KEYS, MuscleAnalysis
    from bioimitation.packdef import state_row_slices
    from bioimitation.vector_env import VectorEnv
    env_id, n = 'MuscleWalkingImitation2D-v0', 8
    env = VectorEnv(env_id, n, precision=64)
    pk = env.pack
    env.reset(ref_index=[3, 11, 19, 27, 35, 43, 51, 59])
    rng = np.random.default_rng(5)
    for _ in range(3):
        env.step(torch.as_tensor(rng.uniform(0, 1, size=(n, env.action_dim)), device=env.device))
    got = env.muscle_analysis(want=KEYS)
    s = env.get_state()
    sl, dim = state_row_slices(pk.ndof, pk.nmuscle, pk.nact, pk.horizon)
    assert dim == env.state_dim
    ma = MuscleAnalysis(env_id, precision=64)
    want = ma.eval(s[:, sl['q']], s[:, sl['u']], s[:, sl['act']], s[:, sl['lce']], want=KEYS)
    for k in KEYS:
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    # a list of envs: their rows, in the list's order
    ids = [6, 1, 4]
    part = env.muscle_analysis(env_ids=ids, want=('length', 'fiber'))
    assert set(part) == {'length', 'fiber'}
    assert torch.equal(part['length'], got['length'][ids]) and torch.equal(part['fiber'], got['fiber'][ids])
    rep = _report_fiber(env, list(range(n)))
    fib = _np(got['fiber'])
    errs = [_rel(fib[:, :, c], rep[:, :, c]) for c in range(5)]
    print('fiber vs the REALIZE report, max rel err (length, velocity, Ft, Ff, Fa)', ' '.join(f'{e:.2e}' for e in errs))
    assert max(errs) < 5e-9, errs
    ma.close()
    env.close()


def test_env_muscle_analysis_is_a_read():
    """Twin envs, one with a muscle_analysis() call between steps: the next
    two steps agree bit for bit, and the realize-cache flags do not move"""
    import torch
    from bioimitation.muscle_analysis import KEYS
    from bioimitation.vector_env import VectorEnv
    env_id, n = 'MuscleWalkingImitation2D-v0', 8
    a, b = (VectorEnv(env_id, n, precision=64, seed=7) for _ in range(2))
    rows = [2, 10, 18, 26, 34, 42, 50, 58]
    rng = np.random.default_rng(6)
    acts = torch.as_tensor(rng.uniform(0, 1, size=(4, n, a.action_dim)), device=a.device)
    for e in (a, b):
        e.reset(ref_index=rows)
        for t in range(2):
            e.step(acts[t])
    flags = a.debug_plane('cache_ok').copy()
    assert flags.any()                     # the steps left a live cache to lose
    a.muscle_analysis(want=KEYS)
    a.muscle_analysis(env_ids=[5, 0], want=('tau',))
    assert (a.debug_plane('cache_ok') == flags).all()
    assert (b.debug_plane('cache_ok') == flags).all()
    for t in (2, 3):
        ra, rb = a.step(acts[t]), b.step(acts[t])
        for x, y, what in zip(ra, rb, ('obs', 'reward', 'done', 'info')):
            assert torch.equal(x, y), (t, what)
    a.close()
    b.close()


def test_torque_model_is_refused():
    from bioimitation._lib import BioimError
    from bioimitation.muscle_analysis import MuscleAnalysis
    from bioimitation.vector_env import VectorEnv
    env_id = 'TorqueWalkingImitation2D-v0'
    ma = MuscleAnalysis(env_id)
    with pytest.raises(BioimError, match='bioim_muscle_eval: the model has no muscles'):
        ma.eval(np.zeros((2, ma.ndof)))
    ma.close()
    env = VectorEnv(env_id, 2)
    env.reset(ref_index=[1, 2])
    with pytest.raises(BioimError, match='bioim_muscle_eval: the model has no muscles'):
        env.muscle_analysis()
    env.close()
