"""Batched body and point kinematics on the GPU.

OpenSim's BodyKinematics and PointKinematics (the kinematics-analysis stage of
the chain scale -> IK -> kinematics analysis -> MuscleAnalysis ->
InverseDynamics -> StaticOptimization) next to the other analyses.  For n
arbitrary states (q, u, q'') it gives, per OpenSim body of the model (one row
per body, ``BodyKinematics.bodies``; ``[3][3]`` is position, velocity,
acceleration, x y z each, in the ground frame):
- ``origin``: the body frame's origin, ``[n][nosbody][3][3]``;
- ``com``: the body's own mass centre (what OpenSim's BodyKinematics reports),
  ``[n][nosbody][3][3]``;
- ``orient``: body-fixed XYZ angles, angular velocity, angular acceleration,
  ``[n][nosbody][3][3]``;
- ``rot``: the rotation body -> ground, row-major, ``[n][nosbody][9]``;
- ``system``: the whole-body mass centre, ``[n][3][3]``;
- ``momentum``: linear momentum and angular momentum about the whole-body mass
  centre, ``[n][2][3]``;
- ``energy``: kinetic and gravitational potential energy, ``[n][2]``;
- ``point``: each of ``points`` (a toe, a marker, a contact sphere's centre:
  ``(body name or 'ground', (x, y, z) in that body's frame)``),
  ``[n][npt][3][3]``.

``local=True`` is OpenSim's ``express_results_in_body_local_frame``: the linear
velocities and accelerations of ``origin`` and ``com`` and the angular ones of
``orient`` are expressed in the body's own frame.  Every call is one launch of
``bioim_body_kin`` (include/bioim.h has the definitions).  There is no CPU
path.  A precision=32 object takes and returns fp32 tensors.

Vectors are in dof order (locked coordinates are not dofs), bodies in the
pack's OpenSim-body order.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._analysis import Analysis, check_rows, check_shape, check_want, ptr as p

NAME = 'body kinematics'

KEYS = ('origin', 'com', 'orient', 'rot', 'system', 'momentum', 'energy', 'point')
DEFAULT_WANT = ('com', 'system')
LOCAL = 1               # include/bioim.h BIOIM_BK_LOCAL
MAX_POINTS = 64         # include/bioim.h BIOIM_BK_MAX_POINTS
GROUND = 'ground'
QUANTITIES = ('pos', 'vel', 'acc')


class Result(dict):
    """``eval``'s result: {key: tensor} plus what ``write_sto`` needs to label
    it (``bodies``, ``local``)."""
    bodies = None
    local = False


def check_points(bodies, points):
    """``points`` (None or a sequence of (body name or 'ground', (x, y, z)))
    as (int32 [npt] OpenSim body indices, -1 = ground; float64 [npt][3])."""
    bodies = list(bodies)
    pts = [] if points is None else list(points)
    if len(pts) > MAX_POINTS:
        raise ValueError(f'body kinematics: {len(pts)} points; one call takes at most {MAX_POINTS}')
    body = np.zeros(len(pts), dtype=np.int32)
    loc = np.zeros((len(pts), 3), dtype=np.float64)
    for i, pt in enumerate(pts):
        try:
            name, xyz = pt
        except (TypeError, ValueError):
            raise ValueError(f'body kinematics: points[{i}] must be (body name, (x, y, z)), got {pt!r}') from None
        if name != GROUND and name not in bodies:
            raise ValueError(f'body kinematics: points[{i}]: unknown body {name!r}; choose from {bodies} or {GROUND!r}')
        check_shape(NAME, xyz, f'points[{i}]\'s location', (3,), batched=False)
        body[i] = -1 if name == GROUND else bodies.index(name)
        loc[i] = np.asarray(xyz, dtype=np.float64)
    return body, loc


def check_args(ndof, bodies, q, u=None, qdd=None, points=None, local=False, want=DEFAULT_WANT):
    """The argument checks of ``BodyKinematics.eval`` (no device needed):
    shapes ``[n][ndof]``, real dtypes, equal row counts, the keys of ``want``,
    the points' bodies (``bodies``: the model's OpenSim body names) and
    locations.  Returns (n, the requested keys, point bodies int32 [npt],
    point locations float64 [npt][3])."""
    want = check_want(NAME, want, KEYS)
    if q is None:
        raise ValueError('body kinematics: q is required')
    pt_body, pt_local = check_points(bodies, points)
    n = check_rows(NAME, (q, 'q', (ndof,)), ((u, 'u', (ndof,)), (qdd, 'qdd', (ndof,))))
    return n, want, pt_body, pt_local


def launch(env, q, u, qdd, pt_body, pt_local, local, want):
    """One ``bioim_body_kin`` launch on ``env``'s handle and stream.  q, u,
    qdd: contiguous tensors on the env's device in its dtype (or None), already
    checked; pt_body / pt_local: ``check_points``'s host arrays.  Returns
    {key: device tensor} for ``want``."""
    import torch
    n, nb, npt = q.shape[0], env.pack.nosbody, int(pt_body.shape[0])
    shapes = dict(origin=(n, nb, 3, 3), com=(n, nb, 3, 3), orient=(n, nb, 3, 3), rot=(n, nb, 9), system=(n, 3, 3),
                  momentum=(n, 2, 3), energy=(n, 2), point=(n, npt, 3, 3))
    bufs = {k: (torch.empty(shapes[k], device=env.device, dtype=env.dtype) if k in want else None) for k in KEYS}
    # (empty tensors have null pointers, which the library reads as outputs not requested)
    live = [k for k in want if bufs[k].numel()]
    if n and live:
        pb = np.ascontiguousarray(pt_body, dtype=np.int32)
        pl = np.ascontiguousarray(pt_local, dtype=np.float64)
        env._bind_stream()
        _lib.check(env._L.bioim_body_kin(env._h, n, p(q), p(u), p(qdd), npt,
                                         pb.ctypes.data_as(C.POINTER(C.c_int32)) if npt else None,
                                         pl.ctypes.data_as(C.POINTER(C.c_double)) if npt else None,
                                         LOCAL if local else 0, *(p(bufs[k]) if k in live else None for k in KEYS)))
    return {k: bufs[k] for k in want}


def columns(bodies):
    """OpenSim's BodyKinematics labels: per body ``<body>_X _Y _Z _Ox _Oy
    _Oz``, then ``center_of_mass_X _Y _Z``."""
    cols = [f'{b}_{a}' for b in bodies for a in ('X', 'Y', 'Z', 'Ox', 'Oy', 'Oz')]
    return cols + [f'center_of_mass_{a}' for a in 'XYZ']


def write_sto(path, time, out, bodies=None, local=None):
    """Write a result as OpenSim's three BodyKinematics storages into the
    directory ``path``: ``task_BodyKinematics_{pos,vel,acc}_global.sto``
    (``_bodyLocal`` for a ``local=True`` result), each a time column and
    ``columns(bodies)``: the bodies' mass centres and body-fixed XYZ angles
    (their rates in vel / acc), then the whole-body mass centre.  Angles are in
    radians (``inDegrees=no``), as the reference tables the envs read.  ``out``:
    ``eval``'s result with 'com', 'orient' and 'system'; a plain dict needs
    ``bodies``.  Returns the three file paths."""
    from . import storage
    bodies = bodies or getattr(out, 'bodies', None)
    local = getattr(out, 'local', False) if local is None else local
    if bodies is None:
        raise ValueError('body kinematics: write_sto needs the body names (eval\'s result carries them)')
    for k in ('com', 'orient', 'system'):
        if k not in out:
            raise ValueError(f'body kinematics: write_sto needs {k!r} in the result (want=("com", "orient", "system"))')
    host = lambda x: x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x)  # noqa: E731
    com, ori, sysm = (host(out[k]).astype(np.float64) for k in ('com', 'orient', 'system'))
    t = np.asarray(time, dtype=np.float64).reshape(-1)
    nb = len(bodies)
    if com.shape != (t.size, nb, 3, 3) or ori.shape != (t.size, nb, 3, 3) or sysm.shape != (t.size, 3, 3):
        raise ValueError(f'body kinematics: write_sto got com {com.shape}, orient {ori.shape}, system {sysm.shape} for '
                         f'{t.size} times and {nb} bodies')
    os.makedirs(path, exist_ok=True)
    files = []
    for j, quantity in enumerate(QUANTITIES):
        per_body = np.concatenate([com[:, :, j, :], ori[:, :, j, :]], axis=2).reshape(t.size, -1)
        data = np.concatenate([t[:, None], per_body, sysm[:, j, :]], axis=1)
        f = os.path.join(path, f'task_BodyKinematics_{quantity}_{"bodyLocal" if local else "global"}.sto')
        storage.write_sto(f, ['time'] + columns(bodies), data, name='BodyKinematics')
        files.append(f)
    return files


class BodyKinematics(Analysis):
    def __init__(self, env_id: str, device: int = 0, precision: int = 64):
        from .obslayout import load_names
        super().__init__(env_id, device, precision)
        pk = self._env.pack
        self.ndof, self.nosbody = pk.ndof, pk.nosbody
        self.bodies = list(load_names(env_id)['bodies'])      # OpenSim body names, in row order

    def index(self, body: str) -> int:
        """Row of a body; ``KeyError`` for an unknown name."""
        if body not in self.bodies:
            raise KeyError(f'body kinematics: no body {body!r}; rows: {self.bodies}')
        return self.bodies.index(body)

    def eval(self, q, u=None, qdd=None, points=None, local=False, want=DEFAULT_WANT):
        """q, u, qdd: [n][ndof] (tensors or arrays, any device / real dtype;
        moved to the env's); points: [(body name or 'ground', (x, y, z))].
        Returns a dict of device tensors for the keys of ``want`` (``KEYS``)."""
        n, want, pt_body, pt_local = check_args(self.ndof, self.bodies, q, u, qdd, points, local, want)
        dev = self._dev
        res = Result(launch(self._env, dev(q), dev(u), dev(qdd), pt_body, pt_local, local, want))
        res.bodies, res.local = self.bodies, bool(local)
        return res

    def write_sto(self, path, time, out):
        return write_sto(path, time, out, bodies=self.bodies)
