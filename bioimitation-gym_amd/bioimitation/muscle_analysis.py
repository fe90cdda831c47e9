"""Batched muscle analysis on the GPU.

OpenSim users expect a MuscleAnalysis next to InverseDynamics.  This is its
batched form on the env's model image.  For n arbitrary states it gives:
- ``length``: the musculotendon path lengths L, ``[n][nmuscle]``;
- ``speed``: the lengthening speeds dL/dt = dL/dq · u, ``[n][nmuscle]``;
- ``dldq``: dL/dq over every dof, ``[n][nmuscle][ndof]``, exact zeros outside
  a muscle's span and on the floating-base dofs;
- ``moment_arms``: OpenSim's moment arms, −dL/dq;
- ``fiber``: fiber length, fiber velocity (m/s), tendon force, fiber force and
  active fiber force at an activation, ``[n][nmuscle][5]`` (``FIBER_COLUMNS``);
- ``tau``: the muscles' generalized force −Σ_m dL_m/dq · Ft_m, ``[n][ndof]``.

``fiber`` and ``tau`` need the activations ``act``.  Without fiber lengths
``lce`` every fiber is first set to its static equilibrium at (act, L)
(OpenSim's ``equilibrateMuscles``).  Every call is one launch of
``bioim_muscle_eval``, which runs the step kernel's own path, equilibrium and
fiber functions.  There is no CPU path.

Vectors are in dof order (locked coordinates are not dofs), muscles in pack
order (``muscle_names``).
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._analysis import Analysis, check_rows, check_want, ptr as p

NAME = 'muscle analysis'

KEYS = ('length', 'speed', 'dldq', 'moment_arms', 'fiber', 'tau')
FIBER_COLUMNS = ('fiber_length', 'fiber_velocity', 'tendon_force', 'fiber_force', 'active_fiber_force')
FIBER_DIM = len(FIBER_COLUMNS)   # include/bioim.h BIOIM_MUSCLE_FIBER_DIM
DEFAULT_WANT = ('length', 'speed', 'dldq')


def check_args(ndof, nmuscle, q, u=None, act=None, lce=None, want=DEFAULT_WANT):
    """The argument checks of ``MuscleAnalysis.eval`` (no device needed):
    shapes ``[n][ndof]`` / ``[n][nmuscle]``, real dtypes, the keys of ``want``
    and the inputs they need.  Returns (n, the requested keys as a tuple)."""
    want = check_want(NAME, want, KEYS)
    if q is None:
        raise ValueError('muscle analysis: q is required')

    n = check_rows(NAME, (q, 'q', (ndof,)), ((u, 'u', (ndof,)), (act, 'act', (nmuscle,)), (lce, 'lce', (nmuscle,))))
    if act is None:
        for k in ('fiber', 'tau'):
            if k in want:
                raise ValueError(f'muscle analysis: {k!r} needs the activations (act)')
    return n, want


def launch(env, q, u, act, lce, want):
    """One ``bioim_muscle_eval`` launch on ``env``'s handle and stream.
    q, u, act, lce: contiguous tensors on the env's device in its dtype (or
    None), already checked.  Returns {key: device tensor} for ``want``."""
    import torch
    n, nd, nm = q.shape[0], env.pack.ndof, env.pack.nmuscle
    new = lambda *s: torch.empty(s, device=env.device, dtype=env.dtype)  # noqa: E731
    if nm == 0:   # a torque model: the library's own refusal (the output given is never written)
        _lib.check(env._L.bioim_muscle_eval(env._h, n, p(q), None, None, None, p(new(1)), None, None, None, None))
    bufs = dict(length=None, speed=None, dldq=None, fiber=None, tau=None)
    if 'length' in want:
        bufs['length'] = new(n, nm)
    if 'speed' in want:
        bufs['speed'] = new(n, nm)
    if 'dldq' in want or 'moment_arms' in want:
        bufs['dldq'] = new(n, nm, nd)
    if 'fiber' in want:
        bufs['fiber'] = new(n, nm, FIBER_DIM)
    if 'tau' in want:
        bufs['tau'] = new(n, nd)
    if n:      # (empty tensors have null pointers, which the library reads as outputs not requested)
        env._bind_stream()
        _lib.check(env._L.bioim_muscle_eval(env._h, n, p(q), p(u), p(act), p(lce), p(bufs['length']),
                                            p(bufs['speed']), p(bufs['dldq']), p(bufs['fiber']), p(bufs['tau'])))
    out = {}
    for k in want:
        out[k] = -bufs['dldq'] if k == 'moment_arms' else bufs[k]
    return out


class MuscleAnalysis(Analysis):
    def __init__(self, env_id: str, device: int = 0, precision: int = 64):
        from .obslayout import load_names
        super().__init__(env_id, device, precision)
        pk = self._env.pack
        self.ndof, self.ncoord, self.nmuscle = pk.ndof, pk.ncoord, pk.nmuscle
        names = load_names(env_id)
        self.muscle_names = list(names.get('muscles') or [])[:pk.nmuscle]
        self.coordinate_names = list(names['coords'])
        self.dof = np.array([pk.coord[c].dof for c in range(pk.ncoord)])

    def eval(self, q, u=None, act=None, lce=None, want=DEFAULT_WANT):
        """q, u: [n][ndof]; act, lce: [n][nmuscle] (tensors or arrays, any
        device / real dtype; moved to the env's).  Returns a dict of device
        tensors for the keys of ``want`` (``KEYS``)."""
        n, want = check_args(self.ndof, self.nmuscle, q, u, act, lce, want)
        dev = self._dev
        return launch(self._env, dev(q), dev(u), dev(act), dev(lce), want)
