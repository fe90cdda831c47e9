"""CPU yardstick of bioim_ik_solve (include/bioim.h): the same damped
Gauss-Newton rule on the oracle's forward kinematics, with a central-difference
Jacobian (h = 1e-6).  Test infrastructure: NumPy + the fp64 C oracle, no GPU.

The marker model of tests/test_ik_pin.py is re-stated here (not imported): a
marker is a point fixed in an OpenSim body's frame, x = p_body + R_body loc on
``Oracle.fk``.  The solver below is the header's rule word for word:

    A = J^T W J + C,  g = J^T W r + C (q - q_target),  f the objective
    mu = 1e-3 max diag A at q0
    per iteration: solve (A + mu I) dq = -g by Cholesky; f_new at q + dq;
      accept if f_new <= f (1 + 64 eps) or max|dq| <= tol:
         max|dq| <= tol -> return (status = iterations)
         else re-form A, g; mu /= 4
      else mu *= 8, same A and g
    every solve counts; max_iter solves done -> status -1; a pivot <= 0 or a
    NaN -> status -2.

Results are cached per (trial, start) so the CPU tests and the GPU tests of
one session share one computation."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps
STRIDE = 6            # the solve tests use every 6th frame of a trial (31 / 40 frames)
CAPS = {'3D': 200, '02905': 400}
TOL = 1e-9
SYNTHETIC = ['MuscleWalkingImitation2D-v0', 'MuscleLockedKneeImitation3D-v0', 'TorqueLockedKneeImitation2D-v0',
             'TorqueWalkingImitation3D-v0']


def load_trial(tag):
    return dict(np.load(os.path.join(HERE, 'golden', f'ik_{tag}.npz'), allow_pickle=False))


class MarkerModel:
    """Marker positions on the oracle's FK of a ModelPack (fp64), in dof order."""

    def __init__(self, oracle_lib, env_id, bodies, locations):
        from bioimitation.obslayout import load_names
        from bioimitation.registry import load_pack
        self.env_id = env_id
        self.pk = load_pack(env_id)
        self.names = load_names(env_id)
        self.orc = oracle_lib.Oracle(self.pk)
        self.bidx = np.array([self.names['bodies'].index(str(b)) for b in bodies])
        self.L = np.asarray(locations, dtype=np.float64)
        self.nm, self.ndof, self.ncoord = len(self.bidx), self.pk.ndof, self.pk.ncoord
        self.dof = np.array([self.pk.coord[c].dof for c in range(self.ncoord)])
        self.free = [c for c in range(self.ncoord) if self.dof[c] >= 0]
        self.default_q = self.qdof(np.array([self.pk.coord[c].default_value for c in range(self.ncoord)]))
        rot = self.names['coord_rotational']
        self.translation = [(int(self.dof[c]), ax)
                            for ax, c in enumerate((self.pk.coord_tx, self.pk.coord_ty, self.pk.coord_tz))
                            if c >= 0 and self.dof[c] >= 0 and not rot[c]]
        self.rotational = np.zeros(self.ndof, dtype=bool)      # by dof
        for c in self.free:
            self.rotational[self.dof[c]] = bool(rot[c])

    def pairs(self):
        """The (osbody name, location) pairs InverseKinematics takes."""
        return [(self.names['bodies'][b], self.L[i]) for i, b in enumerate(self.bidx)]

    def qdof(self, qc):
        qd = np.zeros(self.ndof)
        qd[self.dof[self.free]] = np.asarray(qc)[self.free]
        return qd

    def markers(self, q):
        R, p, _ = self.orc.fk(q)
        return p[self.bidx] + np.einsum('mij,mj->mi', R[self.bidx], self.L)

    def jacobian(self, q, h=1e-6):
        """[nm][3][ndof] by central differences."""
        J = np.zeros((self.nm, 3, self.ndof))
        for d in range(self.ndof):
            qp, qm = q.copy(), q.copy()
            qp[d] += h
            qm[d] -= h
            J[:, :, d] = (self.markers(qp) - self.markers(qm)) / (2 * h)
        return J

    def chain_mask(self):
        """[nm][ndof]: dof d is on marker i's root chain (from the pack's tree)."""
        pk = self.pk
        on = np.zeros((self.nm, self.ndof), dtype=bool)
        dof_cb = {int(self.dof[c]): int(pk.coord[c].cbody) for c in self.free}
        for i, b in enumerate(self.bidx):
            cb, chain = int(pk.osbody[b].cbody), set()
            while cb >= 0:
                chain.add(cb)
                cb = int(pk.cbody[cb].parent)
            for d, c in dof_cb.items():
                on[i, d] = c in chain
        return on

    def cold_start(self, x_exp, w):
        """The default pose with the free translations shifted so the weighted
        marker centroids meet (gaps left out), as InverseKinematics.cold_start."""
        m0 = self.markers(self.default_q)
        ok = np.isfinite(x_exp).all(axis=1)
        wf = w * ok
        shift = (wf[:, None] * (np.where(ok[:, None], x_exp, 0.0) - m0)).sum(0) / max(wf.sum(), np.finfo(float).tiny)
        q0 = self.default_q.copy()
        for d, ax in self.translation:
            q0[d] += shift[ax]
        return q0


def used_weights(x_exp, w):
    return np.where(np.isfinite(x_exp).all(axis=1) & (w > 0), w, 0.0)


def objective(mm, q, x_exp, w, cw=None, qt=None):
    ww = used_weights(x_exp, w)
    r = np.where(ww[:, None] > 0, mm.markers(q) - x_exp, 0.0)
    f = float((ww * (r * r).sum(1)).sum())
    if cw is not None:
        f += float((cw * (q - qt) ** 2).sum())
    return f, r, ww


def normal_equations(mm, q, x_exp, w, cw=None, qt=None):
    f, r, ww = objective(mm, q, x_exp, w, cw, qt)
    J = mm.jacobian(q).reshape(-1, mm.ndof)
    w3 = np.repeat(ww, 3)
    A = J.T @ (w3[:, None] * J)
    g = J.T @ (w3 * r.ravel())
    if cw is not None:
        A = A + np.diag(cw)
        g = g + cw * (q - qt)
    return f, A, g


def solve(mm, x_exp, w, q0, cw=None, qt=None, tol=TOL, max_iter=200):
    """The header's rule.  Returns (q, status)."""
    q = np.array(q0, dtype=np.float64)
    f, A, g = normal_equations(mm, q, x_exp, w, cw, qt)
    if max_iter == 0:
        return q, 0
    if not np.isfinite(f):
        return q, -2
    mu = 1e-3 * A.diagonal().max()
    it = 0
    while True:
        if it >= max_iter:
            return q, -1
        it += 1
        try:
            Lc = np.linalg.cholesky(A + mu * np.eye(mm.ndof))
        except np.linalg.LinAlgError:
            return q, -2
        dq = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, g))
        step = np.abs(dq).max()
        if not np.isfinite(step):
            return q, -2
        fn, An, gn = normal_equations(mm, q + dq, x_exp, w, cw, qt)
        if fn <= f * (1 + 64 * EPS) or step <= tol:
            q, f = q + dq, fn
            if step <= tol:
                return q, it
            A, g, mu = An, gn, mu / 4
        else:
            mu *= 8


def gauss_newton_step(mm, q, x_exp, w, cw=None, qt=None):
    """max |dq| of the undamped Gauss-Newton step at q: 0 at a stationary point."""
    _, A, g = normal_equations(mm, q, x_exp, w, cw, qt)
    return float(np.abs(np.linalg.solve(A, g)).max())


def marker_err(x, x_exp, w):
    """bioim_ik_solve's err: weighted RMS and largest distance over the markers used."""
    ww = used_weights(x_exp, w)
    d2 = np.where(ww > 0, ((x - x_exp) ** 2).sum(1), 0.0)
    return np.array([np.sqrt((ww * d2).sum() / ww.sum()) if ww.sum() > 0 else 0.0, np.sqrt(d2.max())])


_cache = {}


def trial_model(oracle_lib, tag):
    key = ('model', tag)
    if key not in _cache:
        z = load_trial(tag)
        mm = MarkerModel(oracle_lib, str(z['env_id']), z['bodies'], z['locations'])
        assert list(z['coords']) == mm.names['coords']
        _cache[key] = (z, mm)
    return _cache[key]


def trial_frames(tag):
    return np.arange(0, len(load_trial(tag)['q']), STRIDE)


def trial_solution(oracle_lib, tag, start):
    """The yardstick on every STRIDE-th frame of a trial from the 'warm'
    (OpenSim's q) or 'cold' start: dict(frames, q0, q, status), computed once."""
    key = ('solution', tag, start)
    if key not in _cache:
        z, mm = trial_model(oracle_lib, tag)
        frames = trial_frames(tag)
        q0s, qs, st = [], [], []
        for f in frames:
            q0 = mm.qdof(z['q'][f]) if start == 'warm' else mm.cold_start(z['x_exp'][f], z['weights'])
            q, s = solve(mm, z['x_exp'][f], z['weights'], q0, tol=TOL, max_iter=CAPS[tag])
            q0s.append(q0), qs.append(q), st.append(s)
        _cache[key] = dict(frames=frames, q0=np.array(q0s), q=np.array(qs), status=np.array(st))
    return _cache[key]


def noise_floor(oracle_lib, tag):
    """The largest Gauss-Newton step of the yardstick at its own warm solutions."""
    key = ('floor', tag)
    if key not in _cache:
        z, mm = trial_model(oracle_lib, tag)
        sol = trial_solution(oracle_lib, tag, 'warm')
        _cache[key] = max(gauss_newton_step(mm, q, z['x_exp'][f], z['weights'])
                          for f, q, s in zip(sol['frames'], sol['q'], sol['status']) if s >= 0)
    return _cache[key]


def synthetic_model(oracle_lib, env_id):
    """The markers of ik_3D.npz whose bodies the model has, on env_id's model,
    and q* [64][ndof] from the pack's reference rows (spread over the cycle)."""
    key = ('synthetic', env_id)
    if key not in _cache:
        z = load_trial('3D')
        from bioimitation.obslayout import load_names
        have = load_names(env_id)['bodies']
        keep = [i for i, b in enumerate(z['bodies']) if str(b) in have]
        mm = MarkerModel(oracle_lib, env_id, z['bodies'][keep], z['locations'][keep])
        rows = np.linspace(0, mm.pk.nrows - 1, 64).astype(int)
        qstar = np.array([mm.qdof(np.array(mm.pk.ref_q[r][:mm.ncoord])) for r in rows])
        _cache[key] = (mm, z['weights'][keep].copy(), qstar)
    return _cache[key]


def synthetic_start(mm, qstar, seed):
    """q* + U(-0.2, 0.2) on rotations, +- 0.05 m on translations."""
    rng = np.random.default_rng(seed)
    amp = np.where(mm.rotational, 0.2, 0.05)
    return qstar + rng.uniform(-1, 1, size=qstar.shape) * amp
