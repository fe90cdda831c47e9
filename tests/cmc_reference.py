"""Reference for the batched computed muscle control (bioim_cmc), built from the
fp64 oracle alone: a helper of tests/test_cmc_reference.py and
tests/test_gpu_cmc.py, not a test.

The four phases of include/bioim.h, "Computed muscle control":
  1. orc.muscle_paths at q (L0) and at q1 = q + T u (L1, dL/dq), the
     structural zeros of dL/dq set by so_reference.live_mask;
  2. the predictor: a numpy restatement of the oracle's muscle_eval and of its
     semi-implicit muscle update (bioim_oracle.c: muscle_eval,
     solve_fiber_velocity, and the loop after forward_dynamics in substep)
     over orc.curve and the pack's muscle fields;
  3. scipy's BVLS with vector bounds on A = [I; sqrt(lam) B], b = [0; sqrt(lam)
     tau], B[d][m] = -dL_m/dq_d F0_m, x = F / F0, a muscle with an empty force
     range held at its lower bound outside the problem;
  4. the Illinois rules of the header, steps a to e.

Test states (fixed): the oracle reset at reference rows and stepped 3 times
with default_rng U[0, 1] actions (the recipe of test_gpu_body_kinematics.py);
q, u, act, lce from get_state.  Targets: q'' = rng.normal(0, 2), tau =
orc.id_eval(RESIDUAL, q, u, q'').
"""
import ctypes as C
import functools

import numpy as np

from so_reference import live_mask, row_weights

RESIDUAL = 4   # include/bioim.h BIOIM_ID_RESIDUAL
WINDOW, NSUB, FTOL, MAX_ITER = 0.01, 20, 1e-6, 30
NS = 33
FAL, FV, FPE, FSE = 0, 1, 2, 3


class Ref:
    pass


class Muscles:
    """The oracle's muscle model of one pack, restated."""

    def __init__(self, pk, orc):
        self.pk, self.orc = pk, orc
        self._d = C.c_double()
        self._ref = C.byref(self._d)
        self._f = orc.lib.orc_curve

    def curve(self, m, which, x):
        y = self._f(self.orc.pk, m, which, x, self._ref)
        return y, self._d.value

    def fiber_velocity(self, m, afal, beta, rhs):
        """solve_fiber_velocity: (vN, dG/dv)"""
        v, lo, hi = 0.0, -1e6, 1e6
        for _ in range(200):
            y, dy = self.curve(m, FV, v)
            G = afal * y + beta * v - rhs
            dG = afal * dy + beta
            if G > 0:
                hi = v
            else:
                lo = v
            if abs(G) < 1e-13:
                break
            vn = v - G / dG
            if not (vn > lo and vn < hi):
                vn = 0.5 * (lo + hi)
            if abs(vn - v) < 1e-15:
                v = vn
                break
            v = vn
        y, dy = self.curve(m, FV, v)
        return v, afal * dy + beta

    def eval(self, m, a_state, l_state, excitation, L):
        """muscle_eval: (Ft, vce, da/dt, dvce/dlce, clamped)"""
        mu = self.pk.muscle[m]
        a = mu.amin if a_state < mu.amin else (1.0 if a_state > 1.0 else a_state)
        lce = mu.lmin if l_state < mu.lmin else l_state
        w = mu.width
        sq = np.sqrt(lce * lce - w * w)
        cosphi = sq / lce
        lt = L - sq
        fse, dfse = self.curve(m, FSE, lt / mu.lts)
        fal, dfal = self.curve(m, FAL, lce / mu.lopt)
        fpe, dfpe = self.curve(m, FPE, lce / mu.lopt)
        rhs = fse / cosphi - fpe
        vN, dGdv = self.fiber_velocity(m, a * fal, mu.damping, rhs)
        clamped = (l_state <= mu.lmin and vN <= 0) or l_state < mu.lmin
        if clamped:
            vN = 0.0
        fvv, _ = self.curve(m, FV, vN)
        dGdl = (a * dfal * fvv + dfpe) / mu.lopt + dfse / (mu.lts * cosphi * cosphi) + fse * w * w / (sq * sq * sq)
        dvdl = 0.0 if clamped else -(dGdl / dGdv) * mu.lopt * mu.vmax
        u = mu.amin if excitation < mu.amin else (1.0 if excitation > 1.0 else excitation)
        tau = mu.tau_act * (0.5 + 1.5 * a) if u > a else mu.tau_deact / (0.5 + 1.5 * a)
        return mu.fiso * fse, vN * mu.lopt * mu.vmax, (u - a) / tau, dvdl, clamped

    def predict(self, m, a0, l0, L0, L1, e, window=WINDOW, nsub=NSUB):
        """P_m(e): (the end tendon force, the end activation, the end fiber length)"""
        mu = self.pk.muscle[m]
        h = window / nsub
        a, l = a0, l0
        for k in range(nsub):
            L = L0 + (k / nsub) * (L1 - L0)
            _, vce, dadt, dvdl, clamped = self.eval(m, a, l, e, L)
            a += h * dadt
            if not clamped:
                ln = l + h * vce / (1.0 - h * dvdl)
                l = mu.lmin if ln < mu.lmin else ln
        return self.eval(m, a, l, e, L1)[0], a, l

    def bracket(self, m, emin=0.0, emax=1.0):
        amin = self.pk.muscle[m].amin
        el, eh = max(emin, amin), min(emax, 1.0)
        return el, max(eh, el)


def illinois(P, el, eh, Flo, Fhi, Fs, tolF, max_iter=MAX_ITER):
    """Steps a to e of the header on g(e) = P(e)[0] - Fs.  Returns (e, P(e),
    root_status)."""
    a, b, ga, gb = el, eh, Flo - Fs, Fhi - Fs
    side, ev, best = 0, 0, None
    while ev < max_iter:
        c = b - gb * (b - a) / (gb - ga)
        if not (a < c < b):
            c = 0.5 * (a + b)
        pc = P(c)
        gc = pc[0] - Fs
        ev += 1
        if best is None or abs(gc) < best[0]:
            best = (abs(gc), c, pc)
        if abs(gc) <= tolF:
            return c, pc, ev
        if (gc < 0) == (gb < 0):
            b, gb = c, gc
            if side == 1:
                ga *= 0.5
            side = 1
        else:
            a, ga = c, gc
            if side == -1:
                gb *= 0.5
            side = -1
    return best[1], best[2], -1


def paths(r, q, u, q1=None, window=WINDOW):
    """(L0[nm], L1[nm], dL/dq[nm][nd] at q1 with the structural zeros exact)"""
    q1 = q + window * u if q1 is None else q1
    L0 = r.orc.muscle_paths(q, u)[0]
    L1, _, dL = r.orc.muscle_paths(q1, u)
    return L0, L1, np.where(r.live, dL, 0.0)


def ranges(r, act, lce, L0, L1, emin=0.0, emax=1.0, window=WINDOW, nsub=NSUB):
    """per muscle and bracket end (lower, upper): excitation, force, end activation, end fiber length: [nm][2][4]"""
    out = np.zeros((r.pk.nmuscle, 2, 4))
    for m in range(r.pk.nmuscle):
        for k, e in enumerate(r.mus.bracket(m, emin, emax)):
            out[m, k] = (e,) + r.mus.predict(m, act[m], lce[m], L0[m], L1[m], e, window, nsub)
    return out


def allocate(r, rng_, dL, tau, lam):
    """Phase 3: (x[nm], F*[nm], tau_muscle[nd]); x on a bound gives that bound's force itself"""
    from scipy.optimize import lsq_linear
    f0 = np.array([r.pk.muscle[m].fiso for m in range(r.pk.nmuscle)])
    Fmin, Fmax = rng_[:, :, 1].min(1), rng_[:, :, 1].max(1)
    xl, xh = Fmin / f0, Fmax / f0
    B = -(dL * f0[:, None]).T
    free = xh > xl
    x = xl.copy()
    if free.any():
        s = np.sqrt(lam)
        t = tau - B[:, ~free] @ xl[~free]
        A = np.vstack([np.eye(len(f0))[:, free], s[:, None] * B[:, free]])
        b = np.concatenate([np.zeros(len(f0)), s * t])
        sol = lsq_linear(A, b, bounds=(xl[free], xh[free]), method='bvls', tol=1e-14)
        assert sol.status > 0, sol.message
        x[free] = sol.x
    F = np.where(x <= xl, Fmin, np.where(x >= xh, Fmax, x * f0))
    return x, F, B @ x


def solve_state(r, q, u, act, lce, tau, reserve=1.0, q1=None, window=WINDOW, nsub=NSUB, emin=0.0, emax=1.0, ftol=FTOL,
                max_iter=MAX_ITER, roots=True):
    """Every output of bioim_cmc for one state (roots=False: phases 1 to 3 only)."""
    pk, nm = r.pk, r.pk.nmuscle
    L0, L1, dL = paths(r, q, u, q1, window)
    rg = ranges(r, act, lce, L0, L1, emin, emax, window, nsub)
    x, F, tm = allocate(r, rg, dL, tau, row_weights(reserve, pk.ndof))
    out = dict(force_range=rg[:, :, 1].copy(), force=F, tau_muscle=tm, residual=tau - tm, L0=L0, L1=L1)
    if not roots:
        return out
    e, pred, se, rs = np.zeros(nm), np.zeros(nm), np.zeros((nm, 2)), np.zeros(nm, dtype=np.int32)
    for m in range(nm):
        lo_end, hi_end = rg[m]
        up = lo_end[1] <= hi_end[1]
        if F[m] == min(lo_end[1], hi_end[1]):
            end = lo_end if up else hi_end
        elif F[m] == max(lo_end[1], hi_end[1]):
            end = hi_end if up else lo_end
        else:
            P = lambda ee, m=m: r.mus.predict(m, act[m], lce[m], L0[m], L1[m], ee, window, nsub)  # noqa: E731
            ee, pc, rs[m] = illinois(P, lo_end[0], hi_end[0], lo_end[1], hi_end[1], F[m], ftol * pk.muscle[m].fiso,
                                     max_iter)
            end = (ee,) + pc
        e[m], pred[m], se[m] = end[0], end[1], end[2:]
    out.update(excitation=e, predicted=pred, state_end=se, root_status=rs)
    return out


def model(env_id):
    """The pack, the oracle and the restated muscle model of one ID."""
    return _model(env_id)


@functools.lru_cache(maxsize=None)
def _model(env_id):
    import oracle
    from bioimitation.registry import load_pack
    r = Ref()
    r.env_id, r.pk = env_id, load_pack(env_id)
    r.orc = oracle.Oracle(r.pk)
    r.mus = Muscles(r.pk, r.orc)
    r.live = live_mask(r.pk)
    r.f0 = np.array([r.pk.muscle[m].fiso for m in range(r.pk.nmuscle)])
    return r


def draw_states(r, n, seed, steps=3):
    """(q, u [n][nd], act, lce [n][nm], the actions of the last step [n][nact])"""
    from bioimitation.packdef import state_row_slices
    pk, orc = r.pk, r.orc
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, min(pk.nrows - 8, 200), size=n)
    envs = orc.new_envs(n)
    sl, _ = state_row_slices(pk.ndof, pk.nmuscle, pk.nact, pk.horizon)
    st, last = [], []
    for i in range(n):
        orc.reset(envs, i, int(rows[i]))
        for _ in range(steps):
            a = rng.uniform(0, 1, size=pk.nact)
            orc.step(envs, i, a)
        st.append(orc.get_state(envs, i))
        last.append(a)
    st = np.array(st)
    return tuple(st[:, sl[f]].copy() for f in ('q', 'u', 'act', 'lce')) + (np.array(last),)


@functools.lru_cache(maxsize=None)
def _reference(env_id, n=NS):
    """The test states, targets and the reference's outputs on them (read-only, shared)."""
    m = _model(env_id)
    r = Ref()
    r.__dict__.update(m.__dict__)
    r.q, r.u, r.act, r.lce, r.last = draw_states(m, n, seed=41)
    rng = np.random.default_rng(42)
    r.qdd = rng.normal(0.0, 2.0, size=(n, r.pk.ndof))
    r.tau = np.stack([r.orc.id_eval(RESIDUAL, r.q[i], r.u[i], r.qdd[i]) for i in range(n)])
    sols = [solve_state(r, r.q[i], r.u[i], r.act[i], r.lce[i], r.tau[i]) for i in range(n)]
    r.out = {k: np.stack([s[k] for s in sols]) for k in sols[0]}
    for a in list(vars(r).values()) + list(r.out.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


def scaled_errors(r, got, ref):
    """The compared quantities' errors: forces over F0, tau_muscle and residual
    per max(1, |row|), the row being the reference's own for that state"""
    rowmax = lambda a: np.maximum(1.0, np.abs(a).max(axis=1, keepdims=True))  # noqa: E731
    return dict(force_range=(np.abs(got['force_range'] - ref['force_range']) / r.f0[None, :, None]).max(),
                force=(np.abs(got['force'] - ref['force']) / r.f0[None, :]).max(),
                tau_muscle=(np.abs(got['tau_muscle'] - ref['tau_muscle']) / rowmax(ref['tau_muscle'])).max(),
                residual=(np.abs(got['residual'] - ref['residual']) / rowmax(ref['residual'])).max())


@functools.lru_cache(maxsize=None)
def envelope(env_id, n=NS):
    """What one ulp on q moves the compared quantities by, in their own scales
    (the reference against its one-ulp twin, phases 1 to 3): {key: worst}."""
    r = _reference(env_id, n)
    q2 = np.nextafter(r.q, np.inf)
    sols = [solve_state(r, q2[i], r.u[i], r.act[i], r.lce[i], r.tau[i], roots=False) for i in range(n)]
    twin = {k: np.stack([s[k] for s in sols]) for k in sols[0]}
    return scaled_errors(r, twin, r.out)


def bound(env_id, n=NS):
    """The parity bound of tests/test_gpu_cmc.py: 5e-9, or 100 x the envelope where that exceeds 5e-11."""
    env = max(envelope(env_id, n).values())
    return 5e-9 if env <= 5e-11 else 100.0 * env
