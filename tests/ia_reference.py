"""CPU yardstick of bioim_induced_accel (include/bioim.h).  Test
infrastructure: NumPy + the fp64 C oracle, no GPU.

It is not the kernel's recursion.  Per state and contributor one dense KKT
system is solved with ``numpy.linalg.solve``:

    [ M  -J^T ] [ A_c      ]   [ Q_c                          ]
    [ J    0  ] [ lambda_c ] = [ -[c is velocity or total] beta ]

  - M from ``Oracle.mass_bias``; g and c from ``Oracle.id_eval``; dL/dq from
    ``Oracle.muscle_paths``; the per-force contact wrenches from
    ``Oracle.contact``;
  - the station Jacobian J_f, the mass centre's Jacobian and the dofs' Plucker
    columns (which project the contact and external wrenches) are central
    differences of ``Oracle.fk`` poses along the coordinate axes; beta_f and
    the mass centre's velocity term are central second differences along
    q + u t (the composite frames of tests/jr_reference.py);
  - the limit forces are what ``Oracle.id_eval``'s TOTAL leaves beside gravity
    and contact (the GPU tests' states lie strictly inside the limit ranges,
    where they are 0).

Each evaluation is done at step h and at h/2: the result is their Richardson
extrapolation, and |value(h) - value(h/2)| is the yardstick's own noise."""
import numpy as np

import jr_reference as J

H_T = 2e-3      # time step of the second differences (and H_T / 2)
H_Q = 2e-4      # coordinate step of the Jacobians (and H_Q / 2)
GRAVITY, CORIOLIS, TOTAL = 0, 1, 5


class Yardstick:
    def __init__(self, oracle_lib, env_id):
        self.base = b = J.yardstick(oracle_lib, env_id)
        self.pk, self.orc = b.pk, b.orc
        self.nb, self.nd, self.nm, self.nf = b.nb, b.nd, b.nm, b.pk.ncforce
        self.nc = 6 + self.nf + self.nm
        self.mass, self.g = b.mass, b.g
        self.force_body, self.first = b.force_body, b.first
        self.planar = b.pk.coord_tz < 0
        self.nr = 2 if self.planar else 3
        # moved[d][k]: dof d moves composite body k
        self.moved = np.stack([b.sub[b.dof_cb[d]] for d in range(self.nd)])

    def sphere_centre(self, q, f):
        """the ground-frame centre of force f's first sphere"""
        pk = self.pk
        s = [s for s in range(pk.nsphere) if pk.sphere[s].force == f][0]
        Rc, oc = self.base.frames(q)
        k = int(pk.sphere[s].cbody)
        return oc[k] + Rc[k] @ np.array(list(pk.sphere[s].loc))

    def _com(self, q):
        return self.orc.fk(q)[2].copy()

    def _point(self, q, k, loc):
        Rc, oc = self.base.frames(q)
        return oc[k] + Rc[k] @ loc

    def _once(self, q, u, ft, tau_act, ext, kind, cactive, cpoint, ht, hq):
        nd, nf, nr, nc = self.nd, self.nf, self.nr, self.nc
        orc = self.orc
        M, _ = orc.mass_bias(q, u)
        S = self.base._columns(q, hq)                       # [nd][6] Omega3, V3 at the ground origin
        Q = np.zeros((nc, nd))
        Q[0] = orc.id_eval(GRAVITY, q)
        Q[1] = -orc.id_eval(CORIOLIS, q, u)
        held = [f for f in range(nf) if kind == 'point' and cactive is not None and cactive[f]]
        _, w = orc.contact(q, u)
        for f in range(nf):
            if f in held:
                continue
            F, Mo = w[6 * f:6 * f + 3], w[6 * f + 3:6 * f + 6]
            for d in range(nd):
                if self.moved[d, self.force_body[f]]:
                    Q[2 + f, d] = S[d, :3] @ Mo + S[d, 3:] @ F
        # the limit forces: what TOTAL = c - (gravity + contact + limits) leaves (exactly 0 inside the ranges, up to
        # the rounding of this difference)
        Q[2 + nf] = -Q[1] - orc.id_eval(TOTAL, q, u) - Q[0] - orc.contact(q, u)[0]
        if tau_act is not None:
            Q[3 + nf] = tau_act
        if ext is not None:
            for d in range(nd):
                for k in range(self.nb):
                    if self.moved[d, k]:
                        Q[4 + nf, d] += S[d, :3] @ ext[k, 3:] + S[d, 3:] @ ext[k, :3]
        if self.nm and ft is not None:
            dldq = orc.muscle_paths(q, u)[2]
            Q[5 + nf:5 + nf + self.nm] = -ft[:, None] * dldq
        Q[-1] = Q[:-1].sum(0)
        # the mass centre
        Jc = np.zeros((3, nd))
        for d in range(nd):
            e = np.zeros(nd)
            e[d] = hq
            Jc[:, d] = (self._com(q + e) - self._com(q - e)) / (2 * hq)
        cb = (self._com(q + u * ht) - 2 * self._com(q) + self._com(q - u * ht)) / (ht * ht)
        # the held feet
        Jf, beta = np.zeros((nr * len(held), nd)), np.zeros(nr * len(held))
        Rc, oc = self.base.frames(q)
        for j, f in enumerate(held):
            k = self.force_body[f]
            loc = Rc[k].T @ (cpoint[f] - oc[k])
            for d in range(nd):
                e = np.zeros(nd)
                e[d] = hq
                Jf[nr * j:nr * j + nr, d] = ((self._point(q + e, k, loc) - self._point(q - e, k, loc)) / (2 * hq))[:nr]
            beta[nr * j:nr * j + nr] = ((self._point(q + u * ht, k, loc) - 2 * self._point(q, k, loc) +
                                         self._point(q - u * ht, k, loc)) / (ht * ht))[:nr]
        nj = Jf.shape[0]
        K = np.zeros((nd + nj, nd + nj))
        K[:nd, :nd] = M
        K[:nd, nd:] = -Jf.T
        K[nd:, :nd] = Jf
        accel, com, reaction = np.zeros((nc, nd)), np.zeros((nc, 3)), np.zeros((nc, nf, 3))
        for c in range(nc):
            vel = c == 1 or c == nc - 1
            rhs = np.concatenate([Q[c], -beta if vel else np.zeros(nj)])
            x = np.linalg.solve(K, rhs)
            accel[c] = x[:nd]
            com[c] = Jc @ x[:nd] + (cb if vel else 0.0)
            for j, f in enumerate(held):
                reaction[c, f, :nr] = x[nd + nr * j:nd + nr * j + nr]
        return dict(accel=accel, com_accel=com, reaction=reaction, J=Jf, beta=beta, Q=Q)

    # ------------------------------------------------ the model's own feet
    def _own(self, q, u, ht):
        """per force: sum fn_s, sum fn_s P_s and the count of active spheres,
        Hunt-Crossley's normal force restated from the pack (sphere, radius,
        stiffness, dissipation) and the composite frames; the contact point's
        velocity is a central difference of the body-fixed point along q + u t"""
        pk = self.pk
        Rc, oc = self.base.frames(q)
        fs, fP, cnt = np.zeros(self.nf), np.zeros((self.nf, 3)), np.zeros(self.nf, dtype=int)
        for s in range(pk.nsphere):
            sp = pk.sphere[s]
            k, f, r = int(sp.cbody), int(sp.force), sp.radius
            C = oc[k] + Rc[k] @ np.array(list(sp.loc))
            depth = r - C[1]
            if depth <= 0:
                continue
            P = np.array([C[0], C[1] - (r - 0.5 * depth), C[2]])
            loc = Rc[k].T @ (P - oc[k])
            vs = (self._point(q + u * ht, k, loc) - self._point(q - u * ht, k, loc)) / (2 * ht)
            kk = 0.5 * pk.cforce[f].stiffness ** (2.0 / 3.0)
            fH = (4.0 / 3.0) * kk * depth * np.sqrt(r * kk * depth)
            fn = fH * (1.0 + 1.5 * pk.cforce[f].dissipation * -vs[1])
            if not fn > 0:
                continue
            fs[f] += fn
            fP[f] += fn * P
            cnt[f] += 1
        return fs, fP, cnt

    def own_feet(self, q, u):
        """The model's own decision data: (sum fn_s [nf], P_f = sum fn_s P_s /
        sum fn_s [nf][3] (NaN where no sphere is active), active spheres [nf],
        noise of P_f [nf]: |value(h) - value(h/2)|)."""
        fa, Pa, cnt = self._own(q, u, H_T)
        fb, Pb, _ = self._own(q, u, H_T / 2)
        fs, fP = (4.0 * fb - fa) / 3.0, (4.0 * Pb - Pa) / 3.0
        with np.errstate(invalid='ignore', divide='ignore'):
            P = fP / fs[:, None]
            noise = np.abs(Pb / fb[:, None] - Pa / fa[:, None]).max(1)
        return fs, P, cnt, noise

    def eval(self, q, u=None, ft=None, tau_act=None, ext=None, kind='point', cactive=None, cpoint=None):
        """One state.  Returns accel [NC][nd], com_accel [NC][3], reaction
        [NC][nf][3], J, beta, Q (the generalized forces) and noise ({key: max
        |value(h) - value(h/2)|})."""
        q = np.asarray(q, dtype=np.float64)
        u = np.zeros(self.nd) if u is None else np.asarray(u, dtype=np.float64)
        a = self._once(q, u, ft, tau_act, ext, kind, cactive, cpoint, H_T, H_Q)
        b = self._once(q, u, ft, tau_act, ext, kind, cactive, cpoint, H_T / 2, H_Q / 2)
        out, noise = {}, {}
        for k in a:
            out[k] = (4.0 * b[k] - a[k]) / 3.0
            noise[k] = float(np.abs(b[k] - a[k]).max()) if a[k].size else 0.0
        out['noise'] = noise
        return out


_CACHE = {}


def yardstick(oracle_lib, env_id):
    if env_id not in _CACHE:
        _CACHE[env_id] = Yardstick(oracle_lib, env_id)
    return _CACHE[env_id]


def draw_cases(ys, n, seed):
    """n states (tests/jr_reference.py::draw_states: strictly inside every
    limit range, u != 0, state 0 with a foot in Hunt-Crossley contact, state 4
    lowered until a foot stands on two spheres), actuator
    torques (none on the floating base, where they would be external forces
    the momentum identity does not list), external wrenches, and the held feet of the explicit POINT call:
    states cycle through flight, the first foot, the second foot and double
    stance, each held foot at its first sphere's centre."""
    q, u, _ = J.draw_states(ys.base, n, seed)
    # state 4 (a flight state of the explicit call): lowered until one foot stands on two spheres at least, so that
    # the model's own constraint point is a weighted mean of several contact points
    dy = ys.base.dof[ys.pk.coord_ty]
    u[4] *= 0.2
    u[4, dy] = -0.05
    for _ in range(200):
        if ys._own(q[4], u[4], H_T)[2].max() >= 2:
            break
        q[4, dy] -= 0.002
    assert ys.base.inside_limits(q[4], margin=1e-3)
    rng = np.random.default_rng(seed + 1000)
    tau_act = rng.uniform(-20.0, 20.0, size=(n, ys.nd))
    tau_act[:, [d for d in range(ys.nd) if ys.base.parent[ys.base.dof_cb[d]] < 0]] = 0.0   # none on the floating base
    ext = rng.uniform(-30.0, 30.0, size=(n, ys.nb, 6))
    pattern = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], dtype=np.uint8)
    cactive = np.stack([pattern[i % 4][:ys.nf] for i in range(n)])
    cpoint = np.stack([[ys.sphere_centre(q[i], f) for f in range(ys.nf)] for i in range(n)])
    return q, u, tau_act, ext, cactive, cpoint
