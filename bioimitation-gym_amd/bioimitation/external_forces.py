"""Per-env external body forces of the batched step.

OpenSim's ``PrescribedForce`` / ``ExternalForce`` for a batch: up to
``MAX_SLOTS`` force slots per env object.  A slot names an OpenSim body and
the frame its point of application is given in (``'body'``: it moves with the
body; ``'ground'``: fixed in space); both are the same for all envs.  Per env
and slot a row of 9 values, ``ExternalForce``'s column order::

    fx fy fz   force, ground frame (N)
    px py pz   point of application, in the slot's frame (m)
    tx ty tz   torque, ground frame (N m)

lives in one ``(N, K, 9)`` device tensor that every later step, reset,
OsimModel call and every step of a rollout reads at its start
(``bioim_set_external_forces``, include/bioim.h).  The caller writes into the
tensor between steps on the env's stream — like actions, with no host round
trip.  The values are inputs, not state: ``state_rows`` / ``load_state`` /
``clone_envs`` do not carry them, an auto-reset leaves them, and they are not
sanitized.

This module holds the argument checks (no device needed) and the wrench the
analyses take (``ext`` of ``joint_reaction`` / ``induced_accelerations``).
"""
from __future__ import annotations

import numpy as np

NAME = 'external forces'
MAX_SLOTS = 8                       # include/bioim.h BIOIM_MAX_EXT
ROW = 9                             # fx fy fz px py pz tx ty tz
FRAMES = {'body': 0, 'ground': 1}   # include/bioim.h BIOIM_EXT_POINT_BODY / _GROUND


def check_slots(bodies, points, point_in='body'):
    """``points``: a sequence of body names (``bodies``: the model's OpenSim
    body names); ``point_in``: 'body' or 'ground', one for all slots or one per
    slot.  Returns (int32 [K] OpenSim body indices, int32 [K] frame codes)."""
    bodies = list(bodies)
    if isinstance(points, str):
        points = [points]
    try:
        pts = list(points)
    except TypeError:
        raise ValueError(f'{NAME}: points must be a sequence of body names, got {points!r}') from None
    if not pts:
        raise ValueError(f'{NAME}: no slots (set_external_forces(None) removes the forces)')
    if len(pts) > MAX_SLOTS:
        raise ValueError(f'{NAME}: {len(pts)} slots; a handle takes at most {MAX_SLOTS}')
    frames = [point_in] * len(pts) if isinstance(point_in, str) else list(point_in)
    if len(frames) != len(pts):
        raise ValueError(f'{NAME}: point_in has {len(frames)} entries for {len(pts)} slots')
    body = np.zeros(len(pts), dtype=np.int32)
    frame = np.zeros(len(pts), dtype=np.int32)
    for j, (name, fr) in enumerate(zip(pts, frames)):
        if not isinstance(name, str) or name not in bodies:
            raise ValueError(f'{NAME}: points[{j}]: unknown body {name!r}; choose from {bodies}')
        if not isinstance(fr, str) or fr not in FRAMES:
            raise ValueError(f'{NAME}: point_in must be one of {sorted(FRAMES)}, got {fr!r}')
        body[j], frame[j] = bodies.index(name), FRAMES[fr]
    return body, frame


def check_wrench(wrench, n, k, dtype, device):
    """The tensor the launches will read: contiguous ``(n, k, 9)`` of the
    env's dtype on its device (the library takes its pointer as it is)."""
    import torch
    if not isinstance(wrench, torch.Tensor):
        raise ValueError(f'{NAME}: wrench must be a torch tensor, got {type(wrench).__name__}')
    if tuple(wrench.shape) != (n, k, ROW) or wrench.dtype != dtype or wrench.device != device \
            or not wrench.is_contiguous():
        raise ValueError(f'{NAME}: wrench must be a contiguous ({n}, {k}, {ROW}) {dtype} tensor on {device}, got '
                         f'{tuple(wrench.shape)} {wrench.dtype} on {wrench.device}'
                         f'{"" if wrench.is_contiguous() else ", not contiguous"}')
    return wrench


def check_compatible(perturbation, integrator, rk_budget=0):
    """External forces go with the semi-implicit step and without a
    perturbation table (a push is one slot here)."""
    if perturbation is not None:
        raise ValueError(f'{NAME}: apply_perturbations / set_perturbation is set on this env; a push is one force '
                         'slot (remove one of the two)')
    if integrator != 'semi-implicit' or rk_budget:
        raise ValueError(f"{NAME}: integrator='semi-implicit' only (this env runs {integrator!r}"
                         f'{", with an RK budget" if rk_budget else ""})')


def wrench_ground(wrench, os_body, frame, cbody, ncbody, origin, rot):
    """The slots' forces as ``ext`` of the analyses: ``[n][ncbody][6]``
    (fx fy fz mx my mz on each composite body, ground frame, moment about the
    ground origin).  wrench ``[n][K][9]``; os_body / frame: ``check_slots``'s
    arrays; cbody[b]: composite body of OpenSim body b; origin ``[n][nos][3]``
    and rot ``[n][nos][9]`` (row-major, body -> ground): the bodies' frames in
    ground.  All on the tensors' device, nothing read back."""
    import torch
    n = wrench.shape[0]
    ext = torch.zeros((n, ncbody, 6), dtype=wrench.dtype, device=wrench.device)
    for j, (b, fr) in enumerate(zip(os_body.tolist(), frame.tolist())):
        f, p, t = wrench[:, j, 0:3], wrench[:, j, 3:6], wrench[:, j, 6:9]
        if fr == FRAMES['body']:
            p = origin[:, b, :] + torch.matmul(rot[:, b, :].reshape(n, 3, 3), p.unsqueeze(-1)).squeeze(-1)
        cb = int(cbody[b])
        ext[:, cb, 0:3] += f
        ext[:, cb, 3:6] += torch.linalg.cross(p, f) + t
    return ext
