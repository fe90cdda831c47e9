"""Batched induced acceleration analysis on the GPU.

OpenSim's InducedAccelerations next to InverseDynamics, MuscleAnalysis,
StaticOptimization and JointReaction: for n arbitrary states, how much of each
coordinate's acceleration, of the mass centre's acceleration and of each foot's
ground reaction is due to gravity, to the velocity terms, to each contact
force, the limit forces, the caller's actuator and external forces, and to
each single muscle.  One column per contributor
(``InducedAccelerations.contributors``), the last their total:
- ``accel``: ``[n][NC][ndof]``, the coordinate accelerations A_c;
- ``com_accel``: ``[n][NC][3]``, the mass centre's share;
- ``reaction``: ``[n][NC][ncforce][3]``, each foot's share of the ground
  reaction (``kind='point'``; zeros for ``kind='force'`` and feet not held);
- ``cpoint`` / ``cactive``: ``[n][ncforce][3]`` / ``[n][ncforce]``, the
  constraint points and feet that were used;
- ``status``: ``[n]`` int32, 0 ok, -2 a singular or NaN system (zero rows).

``kind='force'`` applies the model's Hunt-Crossley contact as a force
(``total`` is then forward dynamics); ``kind='point'`` is OpenSim's way: every
foot in contact is held by a point constraint and every contributor's share of
the ground reaction is solved for.  The feet and points are the caller's
(``cactive`` with ``cpoint``: a measured ground reaction and centre of
pressure) or the model's own (a foot whose summed normal sphere force exceeds
``force_threshold``, at the force-weighted mean of its spheres' contact
points).  Every call is one launch of ``bioim_induced_accel`` (include/bioim.h
has the definitions).  fp64 only; there is no CPU path.

Vectors are in dof order (locked coordinates are not dofs), bodies in the
pack's composite-body order.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._analysis import Analysis, check_rows, check_want, ptr as p

NAME = 'induced accelerations'

KEYS = ('accel', 'com_accel', 'reaction', 'cpoint', 'cactive', 'status')
DEFAULT_WANT = ('accel',)
KINDS = {'force': 0, 'point': 1}      # include/bioim.h BIOIM_IA_FORCE / _POINT
COM = ('com_x', 'com_y', 'com_z')


def contributor_names(pack, names=None):
    """The contributors in the library's column order: gravity, velocity, one
    per Hunt-Crossley force (the pack's force names, else ``contact_<i>``),
    limits, actuators, external, one per muscle, total."""
    cf = list((names or {}).get('cforces', []) or [])
    if len(cf) != pack.ncforce:
        cf = [f'contact_{i}' for i in range(pack.ncforce)]
    mus = list((names or {}).get('muscles', []) or [])
    if len(mus) != pack.nmuscle:
        mus = [f'muscle_{i}' for i in range(pack.nmuscle)]
    return ['gravity', 'velocity'] + [str(x) for x in cf] + ['limits', 'actuators', 'external'] + \
        [str(x) for x in mus] + ['total']


class Result(dict):
    """``eval``'s result: {key: tensor} plus what ``write_sto`` needs to label
    it (``contributors``, ``coords``, ``kind``)."""
    contributors = None
    coords = None
    kind = 'point'


def check_args(ndof, nmuscle, ncbody, ncforce, q, u=None, ft=None, tau_act=None, ext=None, kind='point',
               cactive=None, cpoint=None, force_threshold=0.0, want=DEFAULT_WANT):
    """The argument checks of ``InducedAccelerations.eval`` (no device needed):
    shapes, real dtypes, the keys of ``want``, ``kind``, ``cactive`` and
    ``cpoint`` together or not at all, a finite ``force_threshold`` >= 0, no
    ``ft`` on a model without muscles.  Returns (n, the requested keys)."""
    want = check_want(NAME, want, KEYS)
    if kind not in KINDS:
        raise ValueError(f'induced accelerations: unknown kind {kind!r}; choose from {tuple(KINDS)}')
    if q is None:
        raise ValueError('induced accelerations: q is required')
    if ft is not None and nmuscle == 0:
        raise ValueError('induced accelerations: ft given, but the model has no muscles')
    if (cactive is None) != (cpoint is None):
        raise ValueError('induced accelerations: cactive and cpoint go together (give both or neither)')
    try:
        thr = float(force_threshold)
    except (TypeError, ValueError):
        raise ValueError(f'induced accelerations: force_threshold must be a number, got {force_threshold!r}') from None
    if not np.isfinite(thr) or thr < 0:
        raise ValueError(f'induced accelerations: force_threshold must be finite and >= 0, got {force_threshold!r}')
    n = check_rows(NAME, (q, 'q', (ndof,)),
                   ((u, 'u', (ndof,)), (ft, 'ft', (nmuscle,)), (tau_act, 'tau_act', (ndof,)), (ext, 'ext', (ncbody, 6)),
                    (cactive, 'cactive', (ncforce,), 'fiub'), (cpoint, 'cpoint', (ncforce, 3))))
    return n, want


def check_env(env):
    if env.precision != 64:
        raise ValueError('induced accelerations: fp64 envs only (M^-1 and a Schur complement on a floating base)')


def launch(env, q, u, ft, tau_act, ext, kind, cactive, cpoint, force_threshold, want):
    """One ``bioim_induced_accel`` launch on ``env``'s handle and stream.  The
    inputs: contiguous float64 tensors on the env's device (``cactive``: uint8)
    or None, already checked.  Returns {key: device tensor} for ``want``."""
    import torch
    pk = env.pack
    n, nd, nf = q.shape[0], pk.ndof, pk.ncforce
    nc = 6 + nf + pk.nmuscle
    shapes = dict(accel=((n, nc, nd), env.dtype), com_accel=((n, nc, 3), env.dtype),
                  reaction=((n, nc, nf, 3), env.dtype), cpoint=((n, nf, 3), env.dtype),
                  cactive=((n, nf), torch.uint8), status=((n,), torch.int32))
    bufs = {k: (torch.empty(shapes[k][0], device=env.device, dtype=shapes[k][1]) if k in want else None) for k in KEYS}
    if n:      # (empty tensors have null pointers, which the library reads as outputs not requested)
        env._bind_stream()
        _lib.check(env._L.bioim_induced_accel(env._h, n, p(q), p(u), p(ft), p(tau_act), p(ext), KINDS[kind],
                                              p(cactive), p(cpoint), float(force_threshold), p(bufs['accel']),
                                              p(bufs['com_accel']), p(bufs['reaction']), p(bufs['cpoint']),
                                              p(bufs['cactive']), p(bufs['status'])))
    return {k: bufs[k] for k in want}


def write_sto(path, time, out, quantity, contributors=None, coords=None):
    """Write one quantity's induced accelerations as an OpenSim storage
    through ``storage.write_sto``: a time column, then one column per
    contributor (OpenSim writes one file per reported quantity).
    ``quantity``: a coordinate (a dof's name or index; from ``out['accel']``)
    or 'com' (three columns per contributor, ``<name>_{x,y,z}``; from
    ``out['com_accel']``).  A plain dict needs ``contributors`` (and ``coords``
    for a coordinate given by name)."""
    from . import storage
    contributors = contributors or getattr(out, 'contributors', None)
    coords = coords or getattr(out, 'coords', None)
    if contributors is None:
        raise ValueError('induced accelerations: write_sto needs the contributor names (eval\'s result carries them)')
    host = lambda x: x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x)  # noqa: E731
    t = np.asarray(time, dtype=np.float64).reshape(-1)
    nc = len(contributors)
    if quantity == 'com':
        if 'com_accel' not in out:
            raise ValueError('induced accelerations: write_sto(\'com\') needs \'com_accel\' in the result')
        a = host(out['com_accel']).astype(np.float64)
        if a.shape != (t.size, nc, 3):
            raise ValueError(f'induced accelerations: write_sto got com_accel {a.shape} for {t.size} times and {nc} '
                             f'contributors')
        cols = [f'{c}_{x}' for c in contributors for x in 'xyz']
        data, name = a.reshape(t.size, -1), 'InducedAccelerations_center_of_mass'
    else:
        if 'accel' not in out:
            raise ValueError('induced accelerations: write_sto of a coordinate needs \'accel\' in the result')
        a = host(out['accel']).astype(np.float64)
        if a.ndim != 3 or a.shape[:2] != (t.size, nc):
            raise ValueError(f'induced accelerations: write_sto got accel {a.shape} for {t.size} times and {nc} '
                             f'contributors')
        if isinstance(quantity, str):
            if coords is None or quantity not in coords:
                raise ValueError(f'induced accelerations: unknown coordinate {quantity!r}; choose from {coords} or \'com\'')
            d, label = list(coords).index(quantity), quantity
        else:
            d = int(quantity)
            if not 0 <= d < a.shape[2]:
                raise ValueError(f'induced accelerations: dof index {d} outside [0, {a.shape[2]})')
            label = coords[d] if coords is not None else f'dof_{d}'
        cols, data, name = list(contributors), a[:, :, d], f'InducedAccelerations_{label}'
    storage.write_sto(path, ['time'] + cols, np.concatenate([t[:, None], data], axis=1), name=name)


def dof_names(pack, names):
    cn = list(names['coords'])
    return [cn[c] for d in range(pack.ndof) for c in range(pack.ncoord) if pack.coord[c].dof == d]


class InducedAccelerations(Analysis):
    def __init__(self, env_id: str, device: int = 0):
        from .obslayout import load_names
        super().__init__(env_id, device, 64)
        pk = self._env.pack
        names = load_names(env_id)
        self.ndof, self.ncbody, self.nmuscle, self.ncforce = pk.ndof, pk.ncbody, pk.nmuscle, pk.ncforce
        self.contributors = contributor_names(pk, names)
        self.coords = dof_names(pk, names)

    def index(self, name: str) -> int:
        """Column of a contributor; ``KeyError`` for an unknown name."""
        if name not in self.contributors:
            raise KeyError(f'induced accelerations: no contributor {name!r}; columns: {self.contributors}')
        return self.contributors.index(name)

    def eval(self, q, u=None, ft=None, tau_act=None, ext=None, kind='point', cactive=None, cpoint=None,
             force_threshold=0.0, want=DEFAULT_WANT):
        """q, u, tau_act: [n][ndof]; ft: [n][nmuscle]; ext: [n][ncbody][6];
        cactive: [n][ncforce] (0 / 1); cpoint: [n][ncforce][3] (tensors or
        arrays, any device / real dtype; moved to the env's).  Returns a dict
        of device tensors for the keys of ``want`` (``KEYS``)."""
        import torch
        n, want = check_args(self.ndof, self.nmuscle, self.ncbody, self.ncforce, q, u, ft, tau_act, ext, kind,
                             cactive, cpoint, force_threshold, want)
        dev = self._dev
        ca = None
        if cactive is not None:
            ca = (dev(cactive, torch.float64) != 0).to(torch.uint8).contiguous()
        res = Result(launch(self._env, dev(q), dev(u), dev(ft), dev(tau_act), dev(ext), kind, ca, dev(cpoint),
                            force_threshold, want))
        res.contributors, res.coords, res.kind = self.contributors, self.coords, kind
        return res

    def write_sto(self, path, time, out, quantity):
        write_sto(path, time, out, quantity, contributors=self.contributors, coords=self.coords)
