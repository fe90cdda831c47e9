"""Batched marker inverse kinematics on the GPU.

OpenSim users run InverseKinematicsTool first: measured marker positions in,
coordinates out; InverseDynamics and StaticOptimization start from its
solution.  This is its batched form on the env's model image.  For n frames it
minimizes, per frame and over the model's dofs,

    Σ_i w_i |x_i(q) − x_exp_i|² + Σ_d c_d (q_d − q_target_d)²

(IKMarkerTasks plus optional IKCoordinateTasks) by damped Gauss-Newton, one
launch of ``bioim_ik_solve`` for all frames (``include/bioim.h`` fixes the
rule).  A marker whose measurement has a NaN in a frame is left out of that
frame.  Coordinate ranges are not enforced.

The results:
- ``q``: the coordinates, ``[n][ndof]`` in dof order (locked coordinates are
  not dofs);
- ``markers``: the model's marker positions at q, ``[n][nm][3]``;
- ``err``: weighted marker RMS and largest marker distance, ``[n][2]``;
- ``jacobian``: ∂x_i/∂q_d at q, ``[n][nm][3][ndof]``, exact zeros where the dof
  is not on the marker's root chain;
- ``status``: per frame the iterations used, −1 if ``max_iter`` was hit, −2 if
  a factorization failed or a NaN came in (no marker and no coordinate task
  left in the frame is such a case), ``[n]``.

fp64 only.  There is no CPU path.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib
from ._analysis import Analysis, check_rows, check_shape, check_want, ptr as p

NAME = 'inverse kinematics'

KEYS = ('q', 'markers', 'err', 'jacobian', 'status')
DEFAULT_WANT = ('q', 'status')
MAX_MARKERS = 64      # BIOIM_IK_MAX_MARKERS (include/bioim.h)
ERR_COLUMNS = ('marker_rms', 'marker_max')


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x, dtype=np.float64)


def check_args(ndof, nm, x_exp, weights=None, q0=None, coord_weight=None, q_target=None, tol=1e-9, max_iter=200,
               want=DEFAULT_WANT):
    """The argument checks of ``InverseKinematics.solve`` (no device needed):
    ``x_exp`` ``[n][nm][3]``, ``weights`` ``[nm]`` finite and non-negative,
    ``q0`` and ``q_target`` ``[n][ndof]``, ``coord_weight`` ``[ndof]`` finite and
    non-negative and given together with ``q_target``, ``tol`` finite and
    non-negative, ``max_iter`` a non-negative integer, the keys of ``want``.
    Returns (n, the requested keys as a tuple)."""
    want = check_want(NAME, want, KEYS)
    if x_exp is None:
        raise ValueError('inverse kinematics: x_exp is required')
    n = check_rows(NAME, (x_exp, 'x_exp', (nm, 3)), ((q0, 'q0', (ndof,)), (q_target, 'q_target', (ndof,))), ' frames')
    if (coord_weight is None) != (q_target is None):
        raise ValueError('inverse kinematics: coord_weight and q_target go together (both or neither)')
    for x, what, m in ((weights, 'weights', nm), (coord_weight, 'coord_weight', ndof)):
        if x is not None:
            check_shape(NAME, x, what, (m,), batched=False)
            v = _host(x)
            if not np.isfinite(v).all() or (v < 0).any():
                raise ValueError(f'inverse kinematics: {what} must be finite and non-negative')
    try:
        tol = float(tol)
    except (TypeError, ValueError):
        raise ValueError('inverse kinematics: tol must be a number') from None
    if not (math.isfinite(tol) and tol >= 0):
        raise ValueError(f'inverse kinematics: tol must be finite and >= 0, got {tol}')
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 0:
        raise ValueError(f'inverse kinematics: max_iter must be an integer >= 0, got {max_iter!r}')
    return n, want


def map_markers(pack, body_names, markers, marker_set=None):
    """Each marker on its composite body: ``markers`` is a sequence of
    ``(osbody name, location in that body's frame)`` pairs or of marker names
    looked up in ``marker_set`` (an ``osim.OsimModel``, its ``markers`` list, or
    the path of an ``.osim`` file).  Returns (names, composite-body index
    int32 ``[nm]``, composite-frame location float64 ``[nm][3]``) through the
    pack's ``osbody[].cbody, R, p``.  ValueError for an unknown body or marker
    name, no marker, or more than ``MAX_MARKERS``."""
    markers = list(markers)
    if not markers:
        raise ValueError('inverse kinematics: no markers given')
    if len(markers) > MAX_MARKERS:
        raise ValueError(f'inverse kinematics: {len(markers)} markers, at most {MAX_MARKERS} (BIOIM_IK_MAX_MARKERS)')
    table = None
    if marker_set is not None:
        if isinstance(marker_set, str):
            from .osim import load_osim
            marker_set = load_osim(marker_set)
        table = {m.name: m for m in getattr(marker_set, 'markers', marker_set)}
    body_names = list(body_names)
    names, cb, loc = [], [], []
    for k, m in enumerate(markers):
        if isinstance(m, str):
            if table is None or m not in table:
                raise ValueError(f'inverse kinematics: marker {m!r} is not in the marker set')
            name, body, l = m, table[m].body, table[m].location
        else:
            try:
                body, l = m
            except (TypeError, ValueError):
                raise ValueError(f'inverse kinematics: marker {k} is neither a name nor a (body, location) pair') from None
            name = f'marker{k}'
        if body not in body_names:
            raise ValueError(f'inverse kinematics: unknown body {body!r} of marker {name!r}; the model has {body_names}')
        try:
            l = np.asarray(l, dtype=np.float64)
        except (TypeError, ValueError):
            l = np.zeros(0)
        if l.shape != (3,) or not np.isfinite(l).all():
            raise ValueError(f'inverse kinematics: the location of marker {name!r} must be 3 finite numbers')
        ob = pack.osbody[body_names.index(body)]
        R = np.array(ob.R[:]).reshape(3, 3)
        names.append(name)
        cb.append(int(ob.cbody))
        loc.append(np.array(ob.p[:]) + R @ l)
    return names, np.array(cb, dtype=np.int32), np.array(loc, dtype=np.float64)


class InverseKinematics(Analysis):
    def __init__(self, env_id: str, markers, marker_set=None, device: int = 0):
        from .obslayout import load_names
        from .registry import load_pack
        names = load_names(env_id)
        pk = load_pack(env_id)
        self.marker_names, cb, loc = map_markers(pk, names['bodies'], markers, marker_set)   # before any device call
        if (cb < 0).any() or (cb >= pk.ncbody).any():
            raise ValueError('inverse kinematics: a marker body lies outside the model')
        import torch
        super().__init__(env_id, device, 64)
        pk = self._env.pack
        self.ndof, self.ncoord, self.nm = pk.ndof, pk.ncoord, len(cb)
        self.coordinate_names = list(names['coords'])
        self.dof = np.array([pk.coord[c].dof for c in range(pk.ncoord)])
        self.default_coords = np.array([pk.coord[c].default_value for c in range(pk.ncoord)])
        free = [c for c in range(pk.ncoord) if self.dof[c] >= 0]
        self.default_q = np.zeros(pk.ndof)
        self.default_q[self.dof[free]] = self.default_coords[free]
        # the free translational coordinates along the ground axes (dof index, axis)
        rot = list(names.get('coord_rotational') or [pk.coord[c].motion == 0 for c in range(pk.ncoord)])
        self.translation = [(int(self.dof[c]), ax) for ax, c in enumerate((pk.coord_tx, pk.coord_ty, pk.coord_tz))
                            if c >= 0 and self.dof[c] >= 0 and not rot[c]]
        self.marker_body, self.marker_loc = cb, loc
        self._cb = torch.as_tensor(cb, device=self.device)
        self._loc = torch.as_tensor(loc, device=self.device).contiguous()
        self._ones = torch.ones(self.nm, device=self.device, dtype=torch.float64)

    def _launch(self, n, x_exp, w, q0, cw, qt, tol, max_iter, want):
        import torch
        env, nd, nm = self._env, self.ndof, self.nm
        new = lambda *s: torch.empty(s, device=self.device, dtype=torch.float64)  # noqa: E731
        bufs = dict(q=new(n, nd), markers=None, err=None, jacobian=None, status=None)
        if 'markers' in want:
            bufs['markers'] = new(n, nm, 3)
        if 'err' in want:
            bufs['err'] = new(n, len(ERR_COLUMNS))
        if 'jacobian' in want:
            bufs['jacobian'] = new(n, nm, 3, nd)
        if 'status' in want:
            bufs['status'] = torch.empty((n,), device=self.device, dtype=torch.int32)
        if n:      # (empty tensors have null pointers, which the library refuses)
            env._bind_stream()
            _lib.check(env._L.bioim_ik_solve(env._h, n, nm, p(self._cb), p(self._loc), p(w), p(x_exp), p(q0), p(cw),
                                             p(qt), float(tol), int(max_iter), p(bufs['q']), p(bufs['markers']),
                                             p(bufs['err']), p(bufs['jacobian']), p(bufs['status'])))
        return {k: bufs[k] for k in want}

    def cold_start(self, x_exp, weights=None):
        """The pack's default pose with the free translational coordinates
        shifted so that the weighted centroid of the model's markers meets
        that of the measured ones, per frame (gaps left out of both).  One
        evaluate-only launch, then tensor arithmetic on the device."""
        import torch
        x = self._dev(x_exp)
        w = self._ones if weights is None else self._dev(weights)
        n = x.shape[0]
        qd = self._dev(self.default_q).reshape(1, -1)
        m0 = self._launch(1, x[:1] if n else x.new_zeros((1, self.nm, 3)), w, qd, None, None, 0.0, 0, ('markers',))
        m0 = m0['markers'][0]
        ok = torch.isfinite(x).all(dim=2)
        wf = w.unsqueeze(0) * ok
        tot = wf.sum(dim=1, keepdim=True).clamp_min(torch.finfo(torch.float64).tiny)
        xe = torch.where(ok.unsqueeze(2), x, torch.zeros_like(x))
        shift = ((wf.unsqueeze(2) * (xe - m0.unsqueeze(0))).sum(dim=1)) / tot
        q0 = qd.repeat(n, 1)
        for d, ax in self.translation:
            q0[:, d] += shift[:, ax]
        return q0

    def solve(self, x_exp, weights=None, q0=None, coord_weight=None, q_target=None, tol=1e-9, max_iter=200,
              want=DEFAULT_WANT):
        """x_exp: [n][nm][3] measured marker positions (ground frame, metres;
        NaN: a gap); weights [nm] (None: all 1); q0 [n][ndof] the start (None:
        ``cold_start``); coord_weight [ndof] with q_target [n][ndof]: the
        coordinate tasks.  Tensors or arrays on any device in any real dtype
        (moved to the env's).  Returns a dict of device tensors for the keys of
        ``want`` (``KEYS``)."""
        n, want = check_args(self.ndof, self.nm, x_exp, weights, q0, coord_weight, q_target, tol, max_iter, want)
        x = self._dev(x_exp)
        w = self._ones if weights is None else self._dev(weights)
        q0 = self.cold_start(x, w) if q0 is None else self._dev(q0)
        return self._launch(n, x, w, q0, self._dev(coord_weight), self._dev(q_target), tol, max_iter, want)

    def evaluate(self, q, x_exp=None, weights=None, want=('markers',)):
        """The forward marker kinematics at q [n][ndof] (the ``max_iter=0``
        call): ``markers`` and ``jacobian``, and with ``x_exp`` also ``err``."""
        import torch
        check_shape(NAME, q, 'q', (self.ndof,))
        q = self._dev(q)
        n = q.shape[0]
        if x_exp is None:
            x_exp = torch.full((n, self.nm, 3), float('nan'), device=self.device, dtype=torch.float64)
        n, want = check_args(self.ndof, self.nm, x_exp, weights, q, None, None, 0.0, 0, want)
        w = self._ones if weights is None else self._dev(weights)
        return self._launch(n, self._dev(x_exp), w, q, None, None, 0.0, 0, want)

    def coordinates(self, q):
        """Dof-ordered q [n][ndof] (tensor or array) as a coordinate-ordered
        array [n][ncoord]; locked coordinates take their pack values."""
        q = _host(q)
        qc = np.tile(self.default_coords, (q.shape[0], 1))
        free = [c for c in range(self.ncoord) if self.dof[c] >= 0]
        qc[:, free] = q[:, self.dof[free]]
        return qc

    def solve_trc(self, path, weights_by_name=None, **kw):
        """``storage.read_trc`` then ``solve``: the file's columns are matched
        to this solver's marker names; ``weights_by_name`` maps names to
        weights (default 1).  Returns (time [n], coordinate-ordered q
        [n][ncoord] as an array, the ``solve`` result): ``['time'] +
        coordinate_names`` and ``column_stack([time, q])`` are the labels and
        table ``storage.write_sto`` takes for the motion file."""
        from .storage import read_trc
        time, names, X = read_trc(path)
        missing = [m for m in self.marker_names if m not in names]
        if missing:
            raise ValueError(f'inverse kinematics: {path} has no columns for the markers {missing}')
        X = X[:, [names.index(m) for m in self.marker_names]]
        wbn = dict(weights_by_name or {})
        unknown = [m for m in wbn if m not in self.marker_names]
        if unknown:
            raise ValueError(f'inverse kinematics: weights for unknown markers {unknown}')
        w = np.array([float(wbn.get(m, 1.0)) for m in self.marker_names])
        want = tuple(kw.pop('want', DEFAULT_WANT))
        out = self.solve(X, weights=w, want=want if 'q' in want else want + ('q',), **kw)
        return time, self.coordinates(out['q']), out

    def write_mot(self, path, time, q_coords):
        """The motion file of ``solve_trc``'s (time, q) through
        ``storage.write_sto`` (radians, ``inDegrees=no``): the IK ``.mot`` that
        ``refmotion.synthesize_reference`` takes."""
        from .storage import write_sto
        write_sto(path, ['time'] + self.coordinate_names, np.column_stack([time, q_coords]), name='Coordinates')
