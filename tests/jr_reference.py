"""CPU yardstick of bioim_joint_reaction (include/bioim.h).  Test
infrastructure: NumPy + the fp64 C oracle, no GPU.

It is not the kernel's recursion.  Newton-Euler is applied to every composite
body on its own, from poses only:

  - the poses come from ``Oracle.fk`` along q(t) = q + u t + q'' t^2 / 2, the
    composite frame rebuilt from an OpenSim body's pose and its placement in
    the composite (``pk.osbody[i].R, p``);
  - the linear part is m c'' by a central second difference of the mass
    centre, the angular part d/dt (R I R^T w) by a central difference of the
    angular momentum at t = +-h/2 (w and R there from the relative rotation of
    two neighbouring samples);
  - gravity; ``Oracle.contact``'s per-force wrenches, assigned to the body
    that carries the force's spheres (``pk.sphere[].cbody / .force``);
  - the muscles' point forces restated from ``pk.pathpt`` (conditional points
    by their range, moving points through ``Oracle.fn``);
  - sums over subtrees from ``pk.cbody[].parent``.

Everything is taken about the true ground origin, then shifted to c_b.  The
dofs' Plucker columns for tau_joint are central differences of the same poses.
Each evaluation is done at step h and at h/2: the result is their Richardson
extrapolation, and |value(h) - value(h/2)| is the yardstick's own noise."""
import numpy as np

H_T = 2e-4      # time step of the acceleration differences (and H_T / 2)
H_Q = 2e-5      # coordinate step of the Plucker columns (and H_Q / 2)


def _vee(A):
    return np.array([A[2, 1] - A[1, 2], A[0, 2] - A[2, 0], A[1, 0] - A[0, 1]]) * 0.5


def _rotvec(A):
    """log of a rotation matrix near the identity, as a vector"""
    w = _vee(A)
    s = np.linalg.norm(w)
    return w if s < 1e-300 else w * (np.arcsin(min(s, 1.0)) / s)


def _exp(v):
    th = np.linalg.norm(v)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    if th < 1e-300:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


class Yardstick:
    def __init__(self, oracle_lib, env_id):
        from bioimitation.registry import load_pack
        self.env_id = env_id
        self.pk = pk = load_pack(env_id)
        self.orc = oracle_lib.Oracle(pk)
        self.nb, self.nd, self.nm, self.nc = pk.ncbody, pk.ndof, pk.nmuscle, pk.ncoord
        self.dof = np.array([pk.coord[c].dof for c in range(pk.ncoord)])
        self.dof_cb = np.zeros(self.nd, dtype=int)
        for c in range(pk.ncoord):
            if self.dof[c] >= 0:
                self.dof_cb[self.dof[c]] = pk.coord[c].cbody
        self.parent = [int(pk.cbody[k].parent) for k in range(self.nb)]
        # sub[b][k]: k lies in b's subtree
        self.sub = np.zeros((self.nb, self.nb), dtype=bool)
        for k in range(self.nb):
            b = k
            while b >= 0:
                self.sub[b, k] = True
                b = self.parent[b]
        self.first = {}
        for i in range(pk.nosbody):
            self.first.setdefault(int(pk.osbody[i].cbody), i)
        self.obR = [np.array(pk.osbody[self.first[k]].R).reshape(3, 3) for k in range(self.nb)]
        self.obp = [np.array(pk.osbody[self.first[k]].p) for k in range(self.nb)]
        self.mass = np.array([pk.cbody[k].mass for k in range(self.nb)])
        self.com = np.array([list(pk.cbody[k].com) for k in range(self.nb)])
        self.Ic = []
        for k in range(self.nb):
            xx, yy, zz, xy, xz, yz = pk.cbody[k].inertia
            self.Ic.append(np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]))
        self.pmb = [np.array(pk.cbody[k].R_mb).reshape(3, 3).T @ np.array(pk.cbody[k].p_mb) for k in range(self.nb)]
        self.g = np.array(list(pk.gravity))
        # the body each contact force acts on
        self.force_body = {}
        for s in range(pk.nsphere):
            f, b = int(pk.sphere[s].force), int(pk.sphere[s].cbody)
            assert self.force_body.setdefault(f, b) == b
        # limited coordinates: (dof, low, up) — inside [low, up] a limit force is exactly 0
        self.limits = [(int(pk.limit[l].dof), pk.limit[l].qlow, pk.limit[l].qup) for l in range(pk.nlimit)
                       if pk.limit[l].dof >= 0]

    # ---------------------------------------------------------------- poses
    def frames(self, q):
        """composite frames (R [nb][3][3], o [nb][3]) from the OpenSim bodies' poses"""
        R, p, _ = self.orc.fk(q)
        Rc = np.stack([R[self.first[k]] @ self.obR[k].T for k in range(self.nb)])
        oc = np.stack([p[self.first[k]] - Rc[k] @ self.obp[k] for k in range(self.nb)])
        return Rc, oc

    def coords(self, q):
        return np.array([q[self.dof[c]] if self.dof[c] >= 0 else self.pk.coord[c].default_value
                         for c in range(self.nc)])

    def inside_limits(self, q, margin=0.0):
        return all(lo + margin <= q[d] <= up - margin for d, lo, up in self.limits)

    # ------------------------------------------------------- inertial part
    def _inertial(self, q, u, qdd, h):
        """[nb][6] (force3, moment3 about the ground origin) of m c'' and dL/dt"""
        at = lambda t: self.frames(q + u * t + 0.5 * qdd * t * t)  # noqa: E731
        (Rm, om), (R0, o0), (Rp, op) = at(-h), at(0.0), at(h)
        W = np.zeros((self.nb, 6))
        for k in range(self.nb):
            c = [o[k] + R[k] @ self.com[k] for R, o in ((Rm, om), (R0, o0), (Rp, op))]
            f = self.mass[k] * (c[2] - 2 * c[1] + c[0]) / (h * h)
            Lh = []
            for Ra, Rb in ((Rm[k], R0[k]), (R0[k], Rp[k])):     # the half-step points
                rv = _rotvec(Rb @ Ra.T)
                Rh = _exp(0.5 * rv) @ Ra
                Lh.append(Rh @ self.Ic[k] @ Rh.T @ (rv / h))
            n = (Lh[1] - Lh[0]) / h
            W[k, :3] = f
            W[k, 3:] = n + np.cross(c[1], f)
        return W

    # ------------------------------------------------------- muscle points
    def muscle_points(self, q, ft):
        """(wrench [nb][6] of the muscles' point forces on each body alone,
        force3 then moment3 about the ground origin; mob [nd]: sum_m Ft_m
        g . dP/dq_d of the moving points' own coordinates)"""
        pk = self.pk
        Rc, oc = self.frames(q)
        qf = self.coords(q)
        W, mob = np.zeros((self.nb, 6)), np.zeros(self.nd)
        for m in range(self.nm):
            mu = pk.muscle[m]
            P, dP, cb, md = [], [], [], []
            for j in range(mu.npt):
                pt = pk.pathpt[mu.pt_off + j]
                if pt.type == 1:   # conditional
                    qc = qf[pt.cond_coord]
                    if qc < pt.range_lo or qc > pt.range_hi:
                        continue
                loc, dloc, mdof = np.array(list(pt.loc)), np.zeros(3), -1
                if pt.type == 2:   # moving
                    ll, dl = loc.copy(), np.zeros(3)
                    for a in range(3):
                        if pt.fn[a] >= 0:
                            cc = pk.fn[pt.fn[a]].coord
                            ll[a], dl[a], _ = self.orc.fn(pt.fn[a], qf[cc])
                            mdof = int(self.dof[cc])
                    Rp = np.array(list(pt.R)).reshape(3, 3)
                    loc, dloc = Rp @ ll + np.array(list(pt.p)), Rp @ dl
                P.append(Rc[pt.cbody] @ loc + oc[pt.cbody])
                dP.append(Rc[pt.cbody] @ dloc)
                cb.append(int(pt.cbody))
                md.append(mdof)
            e = [(P[i + 1] - P[i]) / np.linalg.norm(P[i + 1] - P[i]) for i in range(len(P) - 1)]
            for i in range(len(P)):
                g = (e[i - 1] if i > 0 else 0.0) - (e[i] if i < len(P) - 1 else 0.0)
                f = -ft[m] * g
                W[cb[i], :3] += f
                W[cb[i], 3:] += np.cross(P[i], f)
                if md[i] >= 0:
                    mob[md[i]] += ft[m] * (g @ dP[i])
        return W, mob

    def moving_dofs(self):
        """the dofs that are some moving path point's own coordinate (mdof)"""
        pk, out = self.pk, set()
        for m in range(self.nm):
            for j in range(pk.muscle[m].npt):
                pt = pk.pathpt[pk.muscle[m].pt_off + j]
                if pt.type == 2:
                    out |= {int(self.dof[pk.fn[f].coord]) for f in pt.fn if f >= 0 and self.dof[pk.fn[f].coord] >= 0}
        return sorted(out)

    # ----------------------------------------------------- Plucker columns
    def _columns(self, q, h):
        """S [nd][6] (Omega3, V3 at the ground origin) of each dof on its own body"""
        S = np.zeros((self.nd, 6))
        R0, _ = self.frames(q)
        for d in range(self.nd):
            qp, qm = q.copy(), q.copy()
            qp[d] += h
            qm[d] -= h
            (Rp, op), (Rm, om) = self.frames(qp), self.frames(qm)
            k = self.dof_cb[d]
            om_ = _vee((Rp[k] - Rm[k]) / (2 * h) @ R0[k].T)
            o0 = 0.5 * (op[k] + om[k])
            S[d, :3] = om_
            S[d, 3:] = (op[k] - om[k]) / (2 * h) - np.cross(om_, o0)
        return S

    # ------------------------------------------------------------ the call
    def _once(self, q, u, qdd, ft, ext, contact, ht, hq):
        W = self._inertial(q, u, qdd, ht)
        Rc, oc = self.frames(q)
        c = oc + np.einsum('kij,kj->ki', Rc, self.com)
        for k in range(self.nb):
            fg = self.mass[k] * self.g
            W[k, :3] -= fg
            W[k, 3:] -= np.cross(c[k], fg)
        if contact:
            _, w = self.orc.contact(q, u)
            for f, b in self.force_body.items():
                W[b] -= w[6 * f:6 * f + 6]
        if ext is not None:
            W -= ext
        mw, mob = (self.muscle_points(q, ft) if self.nm and ft is not None else (np.zeros((self.nb, 6)), np.zeros(self.nd)))
        W -= mw
        F = np.stack([W[self.sub[b]].sum(0) for b in range(self.nb)])
        point = np.stack([oc[b] - Rc[b] @ self.pmb[b] for b in range(self.nb)])
        reaction = F.copy()
        reaction[:, 3:] -= np.cross(point, F[:, :3])
        S = self._columns(q, hq)
        tau = np.array([S[d, :3] @ F[self.dof_cb[d], 3:] + S[d, 3:] @ F[self.dof_cb[d], :3] for d in range(self.nd)])
        return dict(W=W, reaction=reaction, point=point, tau_joint=tau, muscle_wrench=mw, mob=mob, R=Rc)

    def eval(self, q, u=None, qdd=None, ft=None, ext=None, contact=True):
        """One state.  Returns {key: value} for W ([nb][6] per body alone),
        reaction ([nb][6], ground frame, about c_b), point, tau_joint,
        muscle_wrench, mob (the moving points' mobility term per dof), R (the
        composite frames), scale (sum_k |W_k|, the size of the terms) and noise
        ({key: max |value(h) - value(h/2)|})."""
        q = np.asarray(q, dtype=np.float64)
        z = np.zeros(self.nd)
        u = z if u is None else np.asarray(u, dtype=np.float64)
        qdd = z if qdd is None else np.asarray(qdd, dtype=np.float64)
        a = self._once(q, u, qdd, ft, ext, contact, H_T, H_Q)
        b = self._once(q, u, qdd, ft, ext, contact, H_T / 2, H_Q / 2)
        out, noise = {}, {}
        for k in ('W', 'reaction', 'tau_joint'):
            out[k] = (4.0 * b[k] - a[k]) / 3.0
            noise[k] = float(np.abs(b[k] - a[k]).max())
        for k in ('point', 'muscle_wrench', 'mob', 'R'):
            out[k] = b[k]
            noise[k] = 0.0
        out['scale'] = float(np.abs(out['W']).sum())
        out['noise'] = noise
        return out


_CACHE = {}


def yardstick(oracle_lib, env_id):
    if env_id not in _CACHE:
        _CACHE[env_id] = Yardstick(oracle_lib, env_id)
    return _CACHE[env_id]


def draw_states(ys, n, seed, contact_state=True):
    """n states of a model strictly inside every limited coordinate's range
    (every limit force is exactly 0 there), u and q'' non-zero.  With
    ``contact_state`` the pelvis height of state 0 is lowered until a foot
    sphere penetrates the ground."""
    pk = ys.pk
    rng = np.random.default_rng(seed)
    Q = np.zeros((n, ys.nd))
    lim = {d: (lo, up) for d, lo, up in ys.limits}
    for c in range(ys.nc):
        d = ys.dof[c]
        if d < 0:
            continue
        lo, up = lim.get(d, (-0.3, 0.3))
        lo, up = max(lo, -0.6), min(up, 0.6)
        Q[:, d] = rng.uniform(lo + 0.05 * (up - lo), up - 0.05 * (up - lo), size=n)
    for c, v in ((pk.coord_tx, 0.4), (pk.coord_ty, 0.95), (pk.coord_tz, 0.1)):
        if c >= 0 and ys.dof[c] >= 0:
            Q[:, ys.dof[c]] = v + rng.uniform(-0.05, 0.05, size=n)
    U = rng.uniform(-1.0, 1.0, size=(n, ys.nd))
    A = rng.uniform(-5.0, 5.0, size=(n, ys.nd))
    if contact_state:
        dy = ys.dof[pk.coord_ty]
        U[0] *= 0.2          # a foot that leaves the ground fast carries no Hunt-Crossley force
        U[0, dy] = -0.1
        Q[0, dy] += 0.3      # from above the ground, down to the first touch
        for _ in range(200):
            if np.abs(ys.orc.contact(Q[0], U[0])[1]).sum() > 0:
                break
            Q[0, dy] -= 0.005
    for i in range(n):
        assert ys.inside_limits(Q[i], margin=1e-3)
    return Q, U, A
