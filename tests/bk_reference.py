"""CPU yardstick of bioim_body_kin (include/bioim.h).  Test infrastructure:
NumPy + the fp64 C oracle, no GPU.

States: the oracle is reset at reference rows and stepped with random actions,
so u and q'' are far from 0.  The yardstick is the oracle's own full report of
that realized state (``Oracle.osim_report``): per OpenSim body the origin's
position, velocity and acceleration, the body-fixed XYZ angles, angular
velocity and acceleration; the system mass centre's p, v, a; and the q'' the
kernel is then given.  Everything else is formed here from that report,
``Oracle.fk``'s rotations and the pack's mass properties:
  - a station r of a body (its mass centre, a point): p + R r, v + w x R r,
    a + al x R r + w x (w x R r);
  - BIOIM_BK_LOCAL: R^T of the velocities and accelerations;
  - momentum: sum m v, and sum R I R^T w + m (c - C) x (v - V) over the
    composite bodies, each carried by the first OpenSim body on it;
  - kinetic energy sum (m v^2 + w . R I R^T w) / 2; potential energy -m g . C.
"""
import numpy as np


class Yardstick:
    def __init__(self, oracle_lib, env_id):
        from bioimitation.obslayout import load_names
        from bioimitation.registry import load_pack
        self.env_id = env_id
        self.pk = pk = load_pack(env_id)
        self.orc = oracle_lib.Oracle(pk)
        self.nc, self.nd, self.nos, self.nb = pk.ncoord, pk.ndof, pk.nosbody, pk.ncbody
        self.bodies = list(load_names(env_id)['bodies'])
        self.free = [c for c in range(pk.ncoord) if pk.coord[c].dof >= 0]
        self.dofs = [int(pk.coord[c].dof) for c in self.free]
        self.os_com = np.array([list(pk.osbody[b].com) for b in range(self.nos)])
        self.first = {}
        for b in range(self.nos):
            self.first.setdefault(int(pk.osbody[b].cbody), b)
        self.mass = np.array([pk.cbody[k].mass for k in range(self.nb)])
        # composite body k's mass centre and inertia in the frame of the OpenSim body that carries it
        self.com_in_first, self.I_in_first = [], []
        for k in range(self.nb):
            ob = pk.osbody[self.first[k]]
            R, p = np.array(ob.R).reshape(3, 3), np.array(ob.p)
            xx, yy, zz, xy, xz, yz = pk.cbody[k].inertia
            I = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])
            self.com_in_first.append(R.T @ (np.array(pk.cbody[k].com) - p))
            self.I_in_first.append(R.T @ I @ R)
        self.g = np.array(list(pk.gravity))

    def draw_states(self, n, seed, steps=3):
        """n realized oracle states: (q, u, qdd [n][ndof], the full reports)."""
        pk, orc = self.pk, self.orc
        rng = np.random.default_rng(seed)
        rows = rng.integers(0, min(pk.nrows - 8, 200), size=n)
        envs = orc.new_envs(n)
        reps = []
        for i in range(n):
            orc.reset(envs, i, int(rows[i]))
            for _ in range(steps):
                orc.step(envs, i, rng.uniform(0, 1, size=pk.nact))
            reps.append(orc.osim_report(envs, i))
        reps = np.array(reps)
        nc = self.nc
        cut = lambda k: reps[:, 2 + k * nc:2 + (k + 1) * nc][:, self.free]  # noqa: E731
        q, u, a = (np.zeros((n, self.nd)) for _ in range(3))
        q[:, self.dofs], u[:, self.dofs], a[:, self.dofs] = cut(0), cut(1), cut(2)
        return q, u, a, reps

    @staticmethod
    def _station(R, p, v, a, w, al, r):
        Rr = R @ r
        return p + Rr, v + np.cross(w, Rr), a + np.cross(al, Rr) + np.cross(w, np.cross(w, Rr))

    def point_indices(self, points):
        return [(-1 if b == 'ground' else self.bodies.index(b), np.array(r, dtype=float)) for b, r in points]

    def eval(self, q, rep, points=(), local=False):
        """Every output of bioim_body_kin for one state from its report."""
        nos, nb = self.nos, self.nb
        ob = 2 + 3 * self.nc
        B = rep[ob:ob + 18 * nos].reshape(nos, 6, 3)      # p v a ang w al
        S = rep[ob + 18 * nos:ob + 18 * nos + 9].reshape(3, 3)
        R, _, _ = self.orc.fk(q)
        out = dict(origin=np.zeros((nos, 3, 3)), com=np.zeros((nos, 3, 3)), orient=np.zeros((nos, 3, 3)),
                   rot=R.reshape(nos, 9).copy(), system=S.copy(), point=np.zeros((len(points), 3, 3)))
        for b in range(nos):
            p, v, a, ang, w, al = B[b]
            out['origin'][b] = p, v, a
            out['com'][b] = self._station(R[b], p, v, a, w, al, self.os_com[b])
            out['orient'][b] = ang, w, al
            if local:
                for key in ('origin', 'com', 'orient'):
                    out[key][b, 1:] = out[key][b, 1:] @ R[b]      # rows R^T x
        for i, (b, r) in enumerate(self.point_indices(points)):
            if b < 0:
                out['point'][i, 0] = r
            else:
                p, v, a, _, w, al = B[b]
                out['point'][i] = self._station(R[b], p, v, a, w, al, r)
        C, V = S[0], S[1]
        lin, ang_m, ke = np.zeros(3), np.zeros(3), 0.0
        for k in range(nb):
            f = self.first[k]
            p, v, a, _, w, al = B[f]
            c, vc, _ = self._station(R[f], p, v, a, w, al, self.com_in_first[k])
            Iw = R[f] @ self.I_in_first[k] @ R[f].T @ w
            lin += self.mass[k] * vc
            ang_m += Iw + self.mass[k] * np.cross(c - C, vc - V)
            ke += 0.5 * (self.mass[k] * vc @ vc + w @ Iw)
        out['momentum'] = np.stack([lin, ang_m])
        out['energy'] = np.array([ke, -self.mass.sum() * self.g @ C])
        return out


def yardstick(oracle_lib, env_id):
    oracle_lib.build()
    return Yardstick(oracle_lib, env_id)
