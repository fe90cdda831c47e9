"""Reference for the batched static optimization (bioim_static_opt), built from
the fp64 oracle alone: a helper of tests/test_static_opt_reference.py and
tests/test_gpu_static_opt.py, not a test.

Per state the rigid-tendon capacity of every muscle (include/bioim.h, "Static
optimization"):
    w    = l_opt sin(alpha_opt)
    l_t  = max(L - l_ts, 0)
    l_m  = max(sqrt(l_t^2 + w^2), l_min)
    cosa = sqrt(l_m^2 - w^2) / l_m
    Fa   = F0 fal(l_m / l_opt) fv(Ldot cosa / (l_opt v_max)) cosa
    Fp   = F0 fpe(l_m / l_opt) cosa
with L, Ldot, dL/dq from orc.muscle_paths and the curves from orc.curve, used
as tests/test_so_pin.py::SOBalance.muscle_force(fiber='rigid') uses them; then
    B[d][m] = -dL_m/dq_d Fa_m,   c_d = -sum_m dL_m/dq_d Fp_m  (0: passive off)
and the box QP
    min sum_m a_m^2 + sum_d lam_d (tau_d - (B a + c)_d)^2,  lo <= a <= hi
solved as the bounded least-squares problem A = [I; sqrt(lam) B],
b = [0; sqrt(lam) (tau - c)] by scipy's BVLS.

dL/dq_d is exactly 0 wherever dof d moves every point of muscle m's path: the
path then moves rigidly (the unit-direction forces along it sum to zero force
and zero moment), unless a moving point's own coordinate is d.  That covers
the dofs outside a muscle's pack span (the floating base among them: "rows no
muscle spans are zero rows of B") and, inside the span, the dofs above a
muscle whose points all sit below them (a knee muscle and the hip dofs; in
LockedKnee3D muscle 18 has no other entry at all).  The oracle forms that sum
in floating point and leaves up to 2.3e-15 there, on every state, where every
other entry reaches at least 7e-3.  Times Fa ~ 8e3 N and a joint or pelvis
residual of 1e3-1e4 N m that noise moves the minimizer by up to 2.9e-8
(LockedKnee3D n = 64: state 54 through the entries outside the span, state 32
through muscle 18's), above the 5e-9 the GPU comparison asks for.  _reference
therefore sets those entries (live_mask, from the pack's structure alone) to
the exact 0 they stand for, as the kernel does, and keeps the oracle's raw
values as dL_raw.  tests/test_static_opt_reference.py pins the noise bound and
prints what keeping it would move.

Test inputs (fixed): rng = default_rng(1); q, u = test_inverse_dynamics._states;
qdd = rng.normal(0, 2, (n, ndof)); tau = orc.id_eval(RESIDUAL, q, u, qdd).
"""
import functools

import numpy as np

RESIDUAL = 4   # include/bioim.h BIOIM_ID_RESIDUAL


class Ref:
    pass


def capacity(pk, orc, q, u):
    """(Fa[nm], Fp[nm], dL[nm][nd], l_t[nm]) of one state"""
    nm = pk.nmuscle
    L, Ld, dL = orc.muscle_paths(q, u)
    Fa, Fp, lts = np.zeros(nm), np.zeros(nm), np.zeros(nm)
    for m in range(nm):
        mu = pk.muscle[m]
        w = mu.lopt * np.sin(mu.alpha_opt)
        lt = max(L[m] - mu.lts, 0.0)
        lm = max(np.sqrt(lt * lt + w * w), mu.lmin)
        cosa = np.sqrt(lm * lm - w * w) / lm
        fal = orc.curve(m, 0, lm / mu.lopt)[0]
        fv = orc.curve(m, 1, Ld[m] * cosa / (mu.lopt * mu.vmax))[0]
        fpe = orc.curve(m, 2, lm / mu.lopt)[0]
        Fa[m] = mu.fiso * fal * fv * cosa
        Fp[m] = mu.fiso * fpe * cosa
        lts[m] = L[m] - mu.lts
    return Fa, Fp, dL, lts


def live_mask(pk):
    """[nm][nd] bool: the entries of dL/dq that are not exactly 0 by
    structure: the dofs on the root paths of some but not all of a muscle's
    path-point bodies, and the dofs of its moving points' own coordinates"""
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
    live = np.zeros((pk.nmuscle, pk.ndof), bool)
    for m in range(pk.nmuscle):
        mu = pk.muscle[m]
        sets, moving = [], set()
        for j in range(mu.npt):
            pt = pk.pathpt[mu.pt_off + j]
            sets.append(path(pt.cbody))
            for f in pt.fn:
                if f >= 0 and pk.fn[f].coord >= 0 and pk.coord[pk.fn[f].coord].dof >= 0:
                    moving.add(pk.coord[pk.fn[f].coord].dof)
        live[m, sorted((set.union(*sets) - set.intersection(*sets)) | moving)] = True
    return live


def row_weights(reserve, nd):
    """lam_d = 1 / reserve_d^2 (reserve: scalar or [nd], inf gives 0)"""
    r = np.broadcast_to(np.asarray(reserve, dtype=np.float64), (nd,))
    with np.errstate(divide='ignore'):
        return 1.0 / (r * r)


def system(Fa, Fp, dL, passive):
    """B[nd][nm], c[nd] of one state"""
    B = -(dL * Fa[:, None]).T
    c = -(dL * Fp[:, None]).sum(0) if passive else np.zeros(dL.shape[1])
    return B, c


def lsq_system(B, c, tau, lam):
    """A = [I; sqrt(lam) B], b = [0; sqrt(lam) (tau - c)]"""
    nm = B.shape[1]
    s = np.sqrt(lam)
    return np.vstack([np.eye(nm), s[:, None] * B]), np.concatenate([np.zeros(nm), s * (tau - c)])


def solve_state(B, c, tau, lam, lo, hi):
    """(a, BVLS iterations) of one state"""
    from scipy.optimize import lsq_linear
    A, b = lsq_system(B, c, tau, lam)
    r = lsq_linear(A, b, bounds=(lo, hi), method='bvls', tol=1e-14)
    assert r.status > 0, r.message
    return r.x, r.nit


def solve(r, tau=None, reserve=1.0, lo=0.0, hi=1.0, passive=False, rows=None):
    """The reference solution on the states `rows` (default: all) of a
    _reference() record: dict of act, tau_muscle, residual, nit."""
    rows = range(len(r.q)) if rows is None else rows
    tau = r.tau if tau is None else tau
    lam = row_weights(reserve, r.pk.ndof)
    out = dict(act=[], tau_muscle=[], residual=[], nit=[])
    for k, i in enumerate(rows):
        B, c = system(r.Fa[i], r.Fp[i], r.dL[i], passive)
        a, nit = solve_state(B, c, tau[k], lam, lo, hi)
        tm = B @ a + c
        out['act'].append(a)
        out['tau_muscle'].append(tm)
        out['residual'].append(tau[k] - tm)
        out['nit'].append(nit)
    return {k: np.array(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _reference(env_id, n):
    """The oracle's values on the test states (read-only, shared)."""
    import oracle
    from bioimitation.registry import load_pack
    from test_inverse_dynamics import _states
    pk = load_pack(env_id)
    orc = oracle.Oracle(pk)
    rng = np.random.default_rng(1)
    nm, nd = pk.nmuscle, pk.ndof
    r = Ref()
    r.pk, r.orc = pk, orc
    r.q, r.u = _states(pk, rng, n)
    r.qdd = rng.normal(0.0, 2.0, size=(n, nd))
    r.tau = np.stack([orc.id_eval(RESIDUAL, r.q[i], r.u[i], r.qdd[i]) for i in range(n)])
    r.Fa, r.Fp, r.dL, r.lt = np.zeros((n, nm)), np.zeros((n, nm)), np.zeros((n, nm, nd)), np.zeros((n, nm))
    for i in range(n):
        r.Fa[i], r.Fp[i], r.dL[i], r.lt[i] = capacity(pk, orc, r.q[i], r.u[i])
    from test_gpu_muscle_analysis import _pack_span
    r.span, r.live = _pack_span(pk), live_mask(pk)
    r.dL_raw = r.dL
    r.dL = np.where(r.live[None], r.dL, 0.0)
    for a in vars(r).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r
