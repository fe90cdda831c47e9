"""Batched joint reaction analysis on the GPU.

OpenSim's JointReaction next to InverseDynamics, MuscleAnalysis and
StaticOptimization: the resultant force and moment every joint carries (the
hip, knee and ankle loads).  For n arbitrary states it gives, per composite
body b of the model (one row per joint, ``JointReaction.joints``):
- ``reaction``: fx fy fz mx my mz of the wrench the parent exerts on b through
  b's inboard joint, the moment about the joint's child-side origin,
  ``[n][ncbody][6]``, expressed in the ground frame, the child's or the
  parent's (``frame``); ``on='parent'`` gives the wrench b exerts on its parent
  instead (the negative, same point);
- ``point``: that origin in the ground frame, ``[n][ncbody][3]``;
- ``tau_joint``: the reaction projected on the dofs, ``[n][ndof]``: what every
  coordinate itself must carry (limit forces, actuators, reserves, a moving
  path point's own-coordinate term);
- ``muscle_wrench``: the muscles' net wrench on each body alone, ground frame,
  about the ground origin, ``[n][ncbody][6]``.

Inputs: q (required), u, q'' (``qdd``), the muscles' tendon forces ``ft``
(``MuscleAnalysis``'s ``fiber[..., 2]``) and external wrenches ``ext`` on the
bodies; ``contact`` adds the model's Hunt-Crossley contact at (q, u).  Every
call is one launch of ``bioim_joint_reaction`` (include/bioim.h has the
definitions).  There is no CPU path.  A precision=32 object takes and returns
fp32 tensors; the kernel computes in fp64 either way.

A joint inside a composite body has no row: welded joints (back, subtalar,
mtp) and locked ones (a locked knee with the ankle behind it) are merged into
one rigid body by the pack, and what they carry is internal to it.

Vectors are in dof order (locked coordinates are not dofs), bodies in the
pack's composite-body order.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._analysis import Analysis, check_rows, check_want, ptr as p

NAME = 'joint reaction'

KEYS = ('reaction', 'point', 'tau_joint', 'muscle_wrench')
DEFAULT_WANT = ('reaction',)
FRAMES = {'ground': 0, 'child': 1, 'parent': 2}   # include/bioim.h BIOIM_JR_GROUND / _CHILD / _PARENT
ON = ('child', 'parent')
CONTACT = 1                                        # include/bioim.h BIOIM_JR_CONTACT
COMPONENTS = ('fx', 'fy', 'fz', 'mx', 'my', 'mz', 'px', 'py', 'pz')


class JointTable:
    """The joints a model has rows for, from its pack and names record (no
    device): ``joints[b]`` the inboard joint of composite body b,
    ``child_bodies[b]`` / ``parent_bodies[b]`` the OpenSim bodies the composite
    frames belong to (the first body of each composite; 'ground' above the
    root), ``inner`` the named joints that lie inside a composite body."""

    def __init__(self, env_id: str):
        from .obslayout import load_names
        from .registry import load_pack
        pk, names = load_pack(env_id), load_names(env_id)
        self.env_id = env_id
        self.ncbody, self.ndof, self.nmuscle = pk.ncbody, pk.ndof, pk.nmuscle
        first = {}
        for b in range(pk.nosbody):
            first.setdefault(int(pk.osbody[b].cbody), names['bodies'][b])
        self.child_bodies = [first[k] for k in range(pk.ncbody)]
        self.parent_bodies = [first[int(pk.cbody[k].parent)] if pk.cbody[k].parent >= 0 else 'ground'
                              for k in range(pk.ncbody)]
        cj = list(names['coord_joints'])
        self.joints = []
        for k in range(pk.ncbody):
            own = [cj[c] for c in range(pk.ncoord) if pk.coord[c].dof >= 0 and pk.coord[c].cbody == k]
            self.joints.append(own[0] if own else self.child_bodies[k] + '_joint')
        # Joints without a row.  The pack names a joint only through its coordinates: a named joint that owns no
        # free coordinate has all of them locked (the coordinate names say which).  A welded joint has no
        # coordinates, so the pack does not carry its name: it is listed by the OpenSim body it holds.
        self.inner = {}
        for c in range(pk.ncoord):
            if cj[c] not in self.joints:
                locked = [names['coords'][d] for d in range(pk.ncoord) if cj[d] == cj[c]]
                self.inner[cj[c]] = (f'its coordinates ({", ".join(locked)}) are locked, so the pack merges its child '
                                     f'into the parent body')
        for b in range(pk.nosbody):
            k = int(pk.osbody[b].cbody)
            if names['bodies'][b] != first[k]:
                self.inner.setdefault(names['bodies'][b] + "'s inboard joint",
                                      f'welded or locked inside composite body {first[k]!r}')

    def index(self, joint: str) -> int:
        """Row of a joint; ``KeyError`` with the reason for a joint inside a
        composite body (or an unknown name)."""
        if joint in self.joints:
            return self.joints.index(joint)
        why = self.inner.get(joint)
        if why is None:
            why = ('the pack names no such joint: it is either a welded joint, which has no coordinates and is merged '
                   'into a composite body (listed by the body it holds: '
                   f'{[k for k in self.inner if k.endswith("inboard joint")]}), or not a joint of this model')
        raise KeyError(f'joint {joint!r} has no row: {why}.  A joint inside a composite body carries only forces '
                       f'internal to that body.  Rows: {self.joints}')

    def columns(self, frame='child', on='child'):
        """OpenSim's JointReaction labels, nine per joint:
        ``<joint>_on_<body>_in_<frame>_{fx,fy,fz,mx,my,mz,px,py,pz}``."""
        check_frame(frame, on)
        cols = []
        for k, j in enumerate(self.joints):
            body = self.child_bodies[k] if on == 'child' else self.parent_bodies[k]
            fr = {'ground': 'ground', 'child': self.child_bodies[k], 'parent': self.parent_bodies[k]}[frame]
            cols += [f'{j}_on_{body}_in_{fr}_{c}' for c in COMPONENTS]
        return cols


class Result(dict):
    """``eval``'s result: {key: tensor} plus what ``write_sto`` needs to label
    it (``table``, ``frame``, ``on``)."""
    table: JointTable = None
    frame = 'child'
    on = 'child'


def check_frame(frame, on):
    if frame not in FRAMES:
        raise ValueError(f'joint reaction: unknown frame {frame!r}; choose from {tuple(FRAMES)}')
    if on not in ON:
        raise ValueError(f'joint reaction: unknown on={on!r}; choose from {ON}')


def check_args(ndof, nmuscle, ncbody, q, u=None, qdd=None, ft=None, ext=None, frame='child', on='child',
               want=DEFAULT_WANT):
    """The argument checks of ``JointReaction.eval`` (no device needed): shapes
    ``[n][ndof]`` / ``[n][nmuscle]`` / ``[n][ncbody][6]``, real dtypes, the keys
    of ``want``, ``frame`` and ``on``, no ``ft`` on a model without muscles.
    Returns (n, the requested keys as a tuple)."""
    want = check_want(NAME, want, KEYS)
    check_frame(frame, on)
    if q is None:
        raise ValueError('joint reaction: q is required')
    if ft is not None and nmuscle == 0:
        raise ValueError('joint reaction: ft given, but the model has no muscles')
    n = check_rows(NAME, (q, 'q', (ndof,)),
                   ((u, 'u', (ndof,)), (qdd, 'qdd', (ndof,)), (ft, 'ft', (nmuscle,)), (ext, 'ext', (ncbody, 6))))
    return n, want


def launch(env, q, u, qdd, ft, ext, contact, frame, on, want):
    """One ``bioim_joint_reaction`` launch on ``env``'s handle and stream.
    q, u, qdd, ft, ext: contiguous tensors on the env's device in its dtype (or
    None), already checked.  Returns {key: device tensor} for ``want``."""
    import torch
    n, nd, nb = q.shape[0], env.pack.ndof, env.pack.ncbody
    new = lambda *s: torch.empty(s, device=env.device, dtype=env.dtype)  # noqa: E731
    shapes = dict(reaction=(n, nb, 6), point=(n, nb, 3), tau_joint=(n, nd), muscle_wrench=(n, nb, 6))
    bufs = {k: (new(*shapes[k]) if k in want else None) for k in KEYS}
    if n:      # (empty tensors have null pointers, which the library reads as outputs not requested)
        env._bind_stream()
        _lib.check(env._L.bioim_joint_reaction(env._h, n, p(q), p(u), p(qdd), p(ft), p(ext),
                                               CONTACT if contact else 0, FRAMES[frame], p(bufs['reaction']),
                                               p(bufs['point']), p(bufs['tau_joint']), p(bufs['muscle_wrench'])))
    out = {k: bufs[k] for k in want}
    if on == 'parent' and 'reaction' in out:
        out['reaction'] = -out['reaction']
    return out


def write_sto(path, time, out, table=None, frame=None, on=None):
    """Write reactions as an OpenSim JointReaction storage through
    ``storage.write_sto``: a time column, then per joint
    ``<joint>_on_<body>_in_<frame>_{fx,fy,fz,mx,my,mz,px,py,pz}``.  ``out``:
    ``eval``'s result with 'reaction' and 'point' ([n][ncbody][6] / [3]); a
    plain dict needs ``table`` (a ``JointTable``), ``frame`` and ``on``."""
    from . import storage
    table = table or getattr(out, 'table', None)
    frame = frame or getattr(out, 'frame', 'child')
    on = on or getattr(out, 'on', 'child')
    if table is None:
        raise ValueError('joint reaction: write_sto needs the joint table (eval\'s result carries it)')
    for k in ('reaction', 'point'):
        if k not in out:
            raise ValueError(f'joint reaction: write_sto needs {k!r} in the result (want=("reaction", "point"))')
    host = lambda x: x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x)  # noqa: E731
    r, pt = host(out['reaction']).astype(np.float64), host(out['point']).astype(np.float64)
    t = np.asarray(time, dtype=np.float64).reshape(-1)
    if r.shape != (t.size, table.ncbody, 6) or pt.shape != (t.size, table.ncbody, 3):
        raise ValueError(f'joint reaction: write_sto got reaction {r.shape}, point {pt.shape} for {t.size} times and '
                         f'{table.ncbody} joints')
    data = np.concatenate([t[:, None], np.concatenate([r, pt], axis=2).reshape(t.size, -1)], axis=1)
    storage.write_sto(path, ['time'] + table.columns(frame, on), data, name='JointReaction')


class JointReaction(Analysis):
    def __init__(self, env_id: str, device: int = 0, precision: int = 64):
        self.table = JointTable(env_id)
        super().__init__(env_id, device, precision)
        pk = self._env.pack
        self.ndof, self.ncbody, self.nmuscle = pk.ndof, pk.ncbody, pk.nmuscle
        self.joints = list(self.table.joints)          # one per composite body; inner joints have no row
        self.inner_joints = dict(self.table.inner)     # {name: why it has no row}

    def index(self, joint: str) -> int:
        return self.table.index(joint)

    def eval(self, q, u=None, qdd=None, ft=None, ext=None, contact=True, frame='child', on='child',
             want=DEFAULT_WANT):
        """q, u, qdd: [n][ndof]; ft: [n][nmuscle]; ext: [n][ncbody][6] (tensors
        or arrays, any device / real dtype; moved to the env's).  Returns a
        dict of device tensors for the keys of ``want`` (``KEYS``)."""
        n, want = check_args(self.ndof, self.nmuscle, self.ncbody, q, u, qdd, ft, ext, frame, on, want)
        dev = self._dev
        res = Result(launch(self._env, dev(q), dev(u), dev(qdd), dev(ft), dev(ext), contact, frame, on, want))
        res.table, res.frame, res.on = self.table, frame, on
        return res

    def write_sto(self, path, time, out):
        write_sto(path, time, out, table=self.table)
