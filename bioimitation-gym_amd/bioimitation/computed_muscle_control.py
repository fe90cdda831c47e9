"""Batched computed muscle control on the GPU.

The muscle envs take excitations.  Static optimization stops one step short
of them: it returns activations under rigid tendons and a force linear in the
activation, while the envs' muscles have compliant tendons, a fiber-length
state and first-order activation dynamics.  This is OpenSim's CMC in batched
form on the env's model image.  Per state and window ``[t, t + T]`` it asks
which excitations make the muscles, integrated through the step's own
activation and contraction dynamics, deliver at ``t + T`` the forces that
produce a wanted generalized force τ:

1. paths: L0 at q, L1 and dL/dq at q1 (``q + T u`` unless given), the path
   length linear in between;
2. the predictor ``P_m(e)``: ``nsub`` muscle substeps at constant excitation e
   from (act, lce), then the tendon force at the end state; its values at the
   two ends of the bracket ``[max(emin, amin_m), min(emax, 1)]`` are the
   muscle's force range;
3. the allocation over ``x_m = F_m / F0_m`` (the sum of squared stresses)

       minimize   Σ_m x_m² + Σ_d λ_d (τ_d − Σ_m (−dL_m/dq_d) F0_m x_m)²
       subject to Fmin_m / F0_m ≤ x_m ≤ Fmax_m / F0_m

   by static optimization's active-set solve (``reserve`` as there: λ =
   1/reserve², ``inf`` leaves the row out);
4. per muscle an Illinois root solve of ``P_m(e) = F*_m`` to ``ftol`` F0
   within ``max_iter`` predictor evaluations.

The results:
- ``excitation``: e*, ``[n][nmuscle]``;
- ``force``: the allocated forces F*, ``[n][nmuscle]``;
- ``force_range``: P_m at the lower and the upper bracket end, ``[n][nmuscle][2]``;
- ``predicted``: P_m(e*), ``[n][nmuscle]``;
- ``state_end``: the predicted activation and fiber length at t + T, ``[n][nmuscle][2]``;
- ``tau_muscle``, ``residual``: the muscles' generalized force and τ minus it, ``[n][ndof]``;
- ``status``: the allocation's passes, −1 / −2 as static optimization's, ``[n]``;
- ``root_status``: predictor evaluations used, 0 for a muscle on a bound of
  its range, −1 if ``max_iter`` was hit, ``[n][nmuscle]``;
- ``tau``: the target itself, ``[n][ndof]``.

Every call is one launch of ``bioim_cmc`` (after one of ``bioim_id_eval`` when
the target is given as accelerations).  fp64 only.  There is no CPU path.

Out of scope: residual actuators on the pelvis (``set_external_forces`` is the
place to apply them), inverting the envs' action smoothing, the torque
models, fp32 and RRA.

Vectors are in dof order (locked coordinates are not dofs), muscles in pack
order (``muscle_names``).
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib
from ._analysis import Analysis, check_reserve, check_rows, check_want, ptr as p, to_device
from .inverse_dynamics import RESIDUAL

NAME = 'computed muscle control'

KEYS = ('excitation', 'force', 'force_range', 'predicted', 'state_end', 'tau_muscle', 'residual', 'status',
        'root_status', 'tau')
DEFAULT_WANT = ('excitation',)
STATE_END_COLUMNS = ('activation', 'fiber_length')


def check_args(ndof, nmuscle, q, u, act, lce, tau=None, qdd=None, q1=None, window=0.01, nsub=None, reserve=1.0,
               emin=0.0, emax=1.0, ftol=1e-6, max_iter=30, want=DEFAULT_WANT):
    """The argument checks of ``ComputedMuscleControl.solve`` (no device
    needed): shapes ``[n][ndof]`` and ``[n][nmuscle]``, real dtypes, exactly
    one of ``qdd`` and ``tau``, a finite positive ``window``, ``nsub`` None or
    an integer ≥ 1, ``max_iter`` an integer ≥ 1, finite ``emin < emax`` and
    ``ftol``, ``reserve`` as static optimization's, the keys of ``want``.
    Returns (n, the requested keys as a tuple, the row weights λ as a float64
    array ``[ndof]``)."""
    want = check_want(NAME, want, KEYS)
    for x, what in ((q, 'q'), (u, 'u'), (act, 'act'), (lce, 'lce')):
        if x is None:
            raise ValueError(f'{NAME}: {what} is required')
    if (qdd is None) == (tau is None):
        raise ValueError(f'{NAME}: give exactly one of qdd and tau')
    n = check_rows(NAME, (q, 'q', (ndof,)), ((u, 'u', (ndof,)), (act, 'act', (nmuscle,)), (lce, 'lce', (nmuscle,)),
                                             (qdd, 'qdd', (ndof,)), (tau, 'tau', (ndof,)), (q1, 'q1', (ndof,))))
    try:
        window, emin, emax, ftol = float(window), float(emin), float(emax), float(ftol)
    except (TypeError, ValueError):
        raise ValueError(f'{NAME}: window, emin, emax and ftol must be numbers') from None
    if not (math.isfinite(window) and window > 0):
        raise ValueError(f'{NAME}: the window must be finite and positive, got {window}')
    if not (math.isfinite(emin) and math.isfinite(emax) and emin < emax):
        raise ValueError(f'{NAME}: the excitation bounds must be finite with emin < emax, got [{emin}, {emax}]')
    if not math.isfinite(ftol):
        raise ValueError(f'{NAME}: ftol must be finite, got {ftol}')
    for v, what, none_ok in ((nsub, 'nsub', True), (max_iter, 'max_iter', False)):
        if v is None and none_ok:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f'{NAME}: {what} must be an integer >= 1, got {v!r}')
    return n, want, check_reserve(NAME, reserve, ndof)


def launch(env, q, u, act, lce, q1, tau, lam, window, nsub, emin, emax, ftol, max_iter, want):
    """One ``bioim_cmc`` launch on ``env``'s handle and stream.  q, u, q1, tau:
    contiguous float64 tensors ``[n][ndof]`` on the env's device (q1 may be
    None), act, lce ``[n][nmuscle]``; lam: float64 ``[ndof]`` there, or None
    for all 1; already checked.  Returns {key: device tensor} for ``want``."""
    import torch
    n, nd, nm = q.shape[0], env.pack.ndof, env.pack.nmuscle
    new = lambda *s: torch.empty(s, device=env.device, dtype=torch.float64)  # noqa: E731
    shapes = dict(force=(n, nm), force_range=(n, nm, 2), predicted=(n, nm), state_end=(n, nm, len(STATE_END_COLUMNS)),
                  tau_muscle=(n, nd), residual=(n, nd))
    bufs = {k: (new(*s) if k in want else None) for k, s in shapes.items()}
    bufs['excitation'] = new(n, nm)
    bufs['status'] = torch.empty((n,), device=env.device, dtype=torch.int32) if 'status' in want else None
    bufs['root_status'] = torch.empty((n, nm), device=env.device, dtype=torch.int32) if 'root_status' in want else None
    if n:      # (empty tensors have null pointers, which the library refuses)
        env._bind_stream()
        _lib.check(env._L.bioim_cmc(env._h, n, p(q), p(u), p(act), p(lce), p(q1), p(tau), p(lam), float(window),
                                    int(nsub), float(emin), float(emax), float(ftol), int(max_iter),
                                    p(bufs['excitation']), p(bufs['force']), p(bufs['force_range']),
                                    p(bufs['predicted']), p(bufs['state_end']), p(bufs['tau_muscle']),
                                    p(bufs['residual']), p(bufs['status']), p(bufs['root_status'])))
    bufs['tau'] = tau
    return {k: bufs[k] for k in want}


def check_env(env):
    """The env-side refusals (the library's own, raised before any launch)."""
    if env.pack.nmuscle == 0:
        raise ValueError(f'{NAME}: the model has no muscles (a torque env)')
    if env.precision != 64:
        raise ValueError(f'{NAME}: fp64 envs only (precision=64); the allocation has no digits in fp32')


def default_nsub(env, window):
    """The step's own substep length carried to ``window``: the handle's
    substep count at the env's 0.01 s step (20), scaled, at least 1."""
    return max(1, int(round(env.pack.nsub * float(window) / 0.01)))


def solve_on(env, q, u, act, lce, tau, qdd, q1, lam, window, nsub, emin, emax, ftol, max_iter, want):
    """The checked arguments of ``solve`` moved to ``env``'s device, the
    inverse-dynamics launch where the target is given as accelerations, then
    ``launch``."""
    import torch
    dev = lambda x: to_device(x, env.device, torch.float64)  # noqa: E731
    check_env(env)
    q, u, act, lce, tau, qdd, q1 = (dev(x) for x in (q, u, act, lce, tau, qdd, q1))
    n = q.shape[0]
    if tau is None:
        tau = torch.empty_like(q)
        if n:
            env._bind_stream()
            _lib.check(env._L.bioim_id_eval(env._h, RESIDUAL, n, p(q), p(u), p(qdd), p(tau)))
    lam_dev = None if (lam == 1.0).all() else dev(lam)
    nsub = default_nsub(env, window) if nsub is None else nsub
    return launch(env, q, u, act, lce, q1, tau, lam_dev, window, nsub, emin, emax, ftol, max_iter, want)


class ComputedMuscleControl(Analysis):
    def __init__(self, env_id: str, device: int = 0):
        from .obslayout import load_names
        super().__init__(env_id, device, 64)
        pk = self._env.pack
        self.ndof, self.ncoord, self.nmuscle = pk.ndof, pk.ncoord, pk.nmuscle
        names = load_names(env_id)
        self.muscle_names = list(names.get('muscles') or [])[:pk.nmuscle]
        self.coordinate_names = list(names['coords'])
        self.dof = np.array([pk.coord[c].dof for c in range(pk.ncoord)])

    def solve(self, q, u, act, lce, tau=None, qdd=None, q1=None, window=0.01, nsub=None, reserve=1.0, emin=0.0,
              emax=1.0, ftol=1e-6, max_iter=30, want=DEFAULT_WANT):
        """q, u: [n][ndof] and act, lce: [n][nmuscle], the state at the
        window's start; exactly one of tau (the target generalized force at
        the window's end) and qdd (accelerations: the target is then
        ``bioim_id_eval(BIOIM_ID_RESIDUAL, q, u, qdd)``, launched first on the
        same stream), [n][ndof]; q1: the coordinates at the window's end
        (default q + window · u); tensors or arrays on any device in any real
        dtype (moved to the env's).  ``nsub``: predictor substeps (default:
        the step's own, 20 at the 0.01 s window).  ``reserve``: scalar or
        [ndof], N·m, ``inf`` allowed.  Returns a dict of device tensors for
        the keys of ``want`` (``KEYS``)."""
        n, want, lam = check_args(self.ndof, self.nmuscle, q, u, act, lce, tau, qdd, q1, window, nsub, reserve,
                                  emin, emax, ftol, max_iter, want)
        return solve_on(self._env, q, u, act, lce, tau, qdd, q1, lam, window, nsub, emin, emax, ftol, max_iter, want)


class CMCDrive:
    """A tracking drive for the muscle envs from computed muscle control, on
    the device (next to ``reflex.ReflexDrive``).

    At construction the reference coordinates and speeds go to the device in
    dof order, with q''_ref = ``np.gradient(u_ref, 0.01, axis=0)``.  A call
    forms, on the device,

        q''* = q''_ref[r] + kv (u_ref[r] − u) + kp (q_ref[r] − q),   r = min(istep + 1, nrows − 1)

    at the envs' current state and returns
    ``venv.computed_muscle_control(qdd=q''*)['excitation']``: an (N, nmuscle)
    action tensor, with no synchronization.  The envs' horizon-5 action
    smoothing sits between this action and the excitation the muscles get, as
    it does for ``ReflexDrive``; it is not inverted.  MusclePalsyImitation3D-v0
    takes the action raw.  The floating base has no muscles: nothing here
    balances the pelvis beyond what the hip and trunk targets do (no residual
    actuators)."""

    def __init__(self, venv, kp=100.0, kv=20.0, reserve=1.0, **solve_kw):
        import torch
        from .packdef import state_row_slices
        pk = venv.pack
        check_env(venv)
        self.venv, self.kp, self.kv, self.reserve, self.solve_kw = venv, float(kp), float(kv), reserve, dict(solve_kw)
        nd = pk.ndof
        self.nrows = pk.nrows
        self.slices, _ = state_row_slices(nd, pk.nmuscle, pk.nact, pk.horizon)
        qref, uref = np.zeros((pk.nrows, nd)), np.zeros((pk.nrows, nd))
        for c in range(pk.ncoord):
            d = pk.coord[c].dof
            if d >= 0:
                qref[:, d] = [pk.ref_q[r][c] for r in range(pk.nrows)]
                uref[:, d] = [pk.ref_u[r][c] for r in range(pk.nrows)]
        aref = np.gradient(uref, 0.01, axis=0)
        dev = dict(device=venv.device, dtype=torch.float64)
        self.qref, self.uref, self.aref = (torch.as_tensor(x, **dev) for x in (qref, uref, aref))

    def target(self, rows):
        """q''* [N][ndof] for the gathered state rows."""
        sl = self.slices
        q, u = rows[:, sl['q']], rows[:, sl['u']]
        r = (rows[:, sl['istep'].start].long() + 1).clamp(max=self.nrows - 1)
        return self.aref[r] + self.kv * (self.uref[r] - u) + self.kp * (self.qref[r] - q)

    def __call__(self):
        """(N, nmuscle) actions for ``venv``'s current state, in its dtype on
        its device."""
        v = self.venv
        rows = v.state_rows()
        out = v.computed_muscle_control(qdd=self.target(rows), reserve=self.reserve, rows=rows, **self.solve_kw)
        return out['excitation'].to(v.dtype)
