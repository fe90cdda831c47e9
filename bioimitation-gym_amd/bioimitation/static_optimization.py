"""Batched static optimization on the GPU.

OpenSim users run StaticOptimization between InverseDynamics and
MuscleAnalysis: given a state and the joint moments a motion needs, which
muscle activations produce them at least effort?  This is its batched form on
the env's model image.  For n arbitrary states it solves, per state,

    minimize   Σ_m a_m² + Σ_d λ_d (τ_d − (B a + c)_d)²
    subject to lo ≤ a_m ≤ hi

with OpenSim's assumptions (``use_muscle_physiology``, rigid tendons):
- ``B[d][m] = −dL_m/dq_d · Fa_m``, Fa the muscle's active capacity (its force
  at a = 1 at the state's fiber length and velocity);
- ``c_d = −Σ_m dL_m/dq_d · Fp_m``, the passive forces, when ``passive`` is on,
  else 0.  Off is the default: OpenSim's balance carries the active force only
  (``tests/test_so_pin.py``);
- the residual ``τ − B a − c`` plays OpenSim's reserve actuators: a reserve of
  optimal torque ``reserve`` N·m on a dof is the weight λ = 1/reserve², and
  ``inf`` leaves the row out.

The results:
- ``act``: the activations, ``[n][nmuscle]``;
- ``tau_muscle``: B a + c, ``[n][ndof]``;
- ``residual``: τ − tau_muscle, ``[n][ndof]``;
- ``capacity``: Fa and Fp, ``[n][nmuscle][2]``;
- ``status``: per state the solver's passes, −1 if the iteration cap was hit,
  −2 if a factorization failed (``act`` is then not the minimizer), ``[n]``;
- ``tau``: the target itself, ``[n][ndof]``.

Every call is one launch of ``bioim_static_opt`` (after one of
``bioim_id_eval`` when the target is given as accelerations), an exact
active-set solve per state.  fp64 only.  There is no CPU path.

Vectors are in dof order (locked coordinates are not dofs), muscles in pack
order (``muscle_names``).
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib
from ._analysis import Analysis, check_reserve, check_rows, check_want, ptr as p, to_device
from .inverse_dynamics import RESIDUAL

NAME = 'static optimization'

KEYS = ('act', 'residual', 'tau_muscle', 'capacity', 'status', 'tau')
DEFAULT_WANT = ('act',)
CAPACITY_COLUMNS = ('active_capacity', 'passive_force')


def check_args(ndof, nmuscle, q, u=None, qdd=None, tau=None, reserve=1.0, lo=0.0, hi=1.0, want=DEFAULT_WANT):
    """The argument checks of ``StaticOptimization.solve`` (no device
    needed): shapes ``[n][ndof]``, real dtypes, exactly one of ``qdd`` and
    ``tau``, ``reserve`` a scalar or ``[ndof]`` of non-negative numbers
    (``inf`` allowed), finite bounds with lo < hi, the keys of ``want``.
    Returns (n, the requested keys as a tuple, the row weights λ as a float64
    array ``[ndof]``)."""
    want = check_want(NAME, want, KEYS)
    if q is None:
        raise ValueError('static optimization: q is required')
    if (qdd is None) == (tau is None):
        raise ValueError('static optimization: give exactly one of qdd and tau')
    n = check_rows(NAME, (q, 'q', (ndof,)), ((u, 'u', (ndof,)), (qdd, 'qdd', (ndof,)), (tau, 'tau', (ndof,))))
    try:
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError('static optimization: the bounds lo and hi must be numbers') from None
    if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
        raise ValueError(f'static optimization: the bounds must be finite with lo < hi, got [{lo}, {hi}]')
    return n, want, check_reserve(NAME, reserve, ndof)


def launch(env, q, u, tau, lam, lo, hi, passive, want):
    """One ``bioim_static_opt`` launch on ``env``'s handle and stream.  q, u,
    tau: contiguous float64 tensors ``[n][ndof]`` on the env's device (u may
    be None); lam: float64 ``[ndof]`` there, or None for all 1; already
    checked.  Returns {key: device tensor} for ``want``."""
    import torch
    n, nd, nm = q.shape[0], env.pack.ndof, env.pack.nmuscle
    new = lambda *s: torch.empty(s, device=env.device, dtype=torch.float64)  # noqa: E731
    bufs = dict(act=new(n, nm), residual=None, tau_muscle=None, capacity=None, status=None)
    if 'residual' in want:
        bufs['residual'] = new(n, nd)
    if 'tau_muscle' in want:
        bufs['tau_muscle'] = new(n, nd)
    if 'capacity' in want:
        bufs['capacity'] = new(n, nm, len(CAPACITY_COLUMNS))
    if 'status' in want:
        bufs['status'] = torch.empty((n,), device=env.device, dtype=torch.int32)
    if n:      # (empty tensors have null pointers, which the library refuses for tau and act)
        env._bind_stream()
        _lib.check(env._L.bioim_static_opt(env._h, n, p(q), p(u), p(tau), p(lam), float(lo), float(hi),
                                           int(bool(passive)), p(bufs['act']), p(bufs['residual']),
                                           p(bufs['tau_muscle']), p(bufs['capacity']), p(bufs['status'])))
    bufs['tau'] = tau
    return {k: bufs[k] for k in want}


class StaticOptimization(Analysis):
    def __init__(self, env_id: str, device: int = 0):
        from .obslayout import load_names
        super().__init__(env_id, device, 64)
        pk = self._env.pack
        self.ndof, self.ncoord, self.nmuscle = pk.ndof, pk.ncoord, pk.nmuscle
        names = load_names(env_id)
        self.muscle_names = list(names.get('muscles') or [])[:pk.nmuscle]
        self.coordinate_names = list(names['coords'])
        self.dof = np.array([pk.coord[c].dof for c in range(pk.ncoord)])

    def solve(self, q, u=None, qdd=None, tau=None, reserve=1.0, lo=0.0, hi=1.0, passive=False, want=DEFAULT_WANT):
        """q, u: [n][ndof]; exactly one of qdd (the accelerations: the target
        is then ``bioim_id_eval(BIOIM_ID_RESIDUAL, q, u, qdd)``, launched first
        on the same stream) and tau (the target itself), [n][ndof]; tensors or
        arrays on any device in any real dtype (moved to the env's).
        ``reserve``: scalar or [ndof], N·m, ``inf`` allowed.  Returns a dict
        of device tensors for the keys of ``want`` (``KEYS``)."""
        n, want, lam = check_args(self.ndof, self.nmuscle, q, u, qdd, tau, reserve, lo, hi, want)
        return solve_on(self._env, q, u, qdd, tau, lam, lo, hi, passive, want)


def solve_on(env, q, u, qdd, tau, lam, lo, hi, passive, want):
    """The checked arguments of ``solve`` moved to ``env``'s device, the
    inverse-dynamics launch where the target is given as accelerations, then
    ``launch``."""
    import torch
    dev = lambda x: to_device(x, env.device, torch.float64)  # noqa: E731
    check_env(env)
    q, u, qdd, tau = dev(q), dev(u), dev(qdd), dev(tau)
    n = q.shape[0]
    if tau is None:
        tau = torch.empty_like(q)
        if n:
            uu = u if u is not None else torch.zeros_like(q)
            env._bind_stream()
            _lib.check(env._L.bioim_id_eval(env._h, RESIDUAL, n, p(q), p(uu), p(qdd), p(tau)))
    lam_dev = None if (lam == 1.0).all() else dev(lam)
    return launch(env, q, u, tau, lam_dev, lo, hi, passive, want)


def check_env(env):
    """The env-side refusals (the library's own, raised before any launch)."""
    if env.pack.nmuscle == 0:
        raise ValueError('static optimization: the model has no muscles (a torque env)')
    if env.precision != 64:
        raise ValueError('static optimization: fp64 envs only (precision=64); the solve has no digits in fp32')
