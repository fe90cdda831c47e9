"""Reference-motion tables the imitation envs read.

Every env loads ``*_reference_data/task_Kinematics_{q,u}.sto`` and
``task_BodyKinematics_{pos,vel}_global.sto``
(``muscle_walking_imitation_env2D.py:46-53``), produced upstream by an
OpenSim AnalyzeTool run (``data/3D/walking_reference_data/setup_ka.xml``:
Kinematics + BodyKinematics over the IK ``.mot`` with a 6 Hz low-pass).
Those ``.sto`` files are git-ignored in the reference (``.gitignore:18``) and
absent, and the 2D recipe's input (``data/2D/walking_reference_data/setup_ka.xml:70``,
``healthy_gait.sto``) is absent too.

:func:`synthesize_2d_walking` therefore regenerates a 2D walking reference from
the sagittal columns of the shipped 3D IK (``data/3D/inverse_kinematics/task_InverseKinematics.mot``):
6 Hz zero-phase low-pass, degrees to radians (both models share the gait2392
sign conventions: knee flexion negative), pelvis height shifted so the lowest
contact sphere touches the ground at the gait's deepest point, speeds from
the spline derivative, and BodyKinematics (body mass-center positions) from
this package's own forward kinematics.  The result is committed under
``bioimitation/data/2D/walking_reference_data``.
"""
from __future__ import annotations

import math
import os

import numpy as np

from .modelpack import REF_BODIES, raw_forward_kinematics
from .storage import read_sto, resample_linear, write_sto

SAGITTAL_MAP_2D = [  # 2D coordinate <- (3D IK column, sign)
    ('pelvis_tilt', 'pelvis_tilt', 1.0), ('pelvis_tx', 'pelvis_tx', 1.0), ('pelvis_ty', 'pelvis_ty', 1.0),
    ('hip_flexion_r', 'hip_flexion_r', 1.0), ('knee_angle_r', 'knee_angle_r', 1.0),
    ('ankle_angle_r', 'ankle_angle_r', 1.0), ('hip_flexion_l', 'hip_flexion_l', 1.0),
    ('knee_angle_l', 'knee_angle_l', 1.0), ('ankle_angle_l', 'ankle_angle_l', 1.0),
]


def _lowpass(x, dt, fc=6.0):
    from scipy.signal import butter, filtfilt
    b, a = butter(4, fc / (0.5 / dt))
    return filtfilt(b, a, x, axis=0, padtype='odd', padlen=min(3 * max(len(a), len(b)), x.shape[0] - 1))


def _spline_derivative(t, x):
    from scipy.interpolate import CubicSpline
    return CubicSpline(t, x, axis=0)(t, 1)


def lowest_sphere_y(model, qval):
    poses, _ = raw_forward_kinematics(model, qval)
    low = math.inf
    for s in model.spheres:
        R, p = poses[s.body]
        low = min(low, (R @ s.loc + p)[1] - s.radius)
    return low


def body_com_table(model, coord_order, q):
    """Mass-center positions (rows, len(bodies)+1, 3) in REF-style order:
    every body of the model then center_of_mass."""
    bodies = list(model.body_order)
    out = np.zeros((q.shape[0], len(bodies) + 1, 3))
    rot = np.zeros((q.shape[0], len(bodies), 3))
    for r in range(q.shape[0]):
        qv = dict(zip(coord_order, q[r]))
        poses, com = raw_forward_kinematics(model, qv)
        for k, b in enumerate(bodies):
            R, p = poses[b]
            out[r, k] = R @ model.bodies[b].com + p
            # body-fixed XYZ angles (BodyKinematics _Ox/_Oy/_Oz)
            rot[r, k] = [math.atan2(-R[1, 2], R[2, 2]), math.asin(max(-1.0, min(1.0, R[0, 2]))),
                         math.atan2(-R[0, 1], R[0, 0])]
        out[r, -1] = com
    return bodies, out, rot


def synthesize_reference(model, ik_mot_path, out_dir, coord_map=None, penetration=0.01, dt=0.01):
    """The AnalyzeTool recipe of ``setup_ka.xml`` (Kinematics + BodyKinematics
    over the IK ``.mot``, 6 Hz low-pass, ``data/3D/walking_reference_data/setup_ka.xml:72-76``)
    restated on this package's FK, plus one calibration the recipe does not
    have: pelvis_ty is shifted so the deepest contact-sphere penetration over
    the trial is ``penetration`` (the shipped IK puts the feet 2-9 cm into the
    ground plane of the predictive model), and pelvis_tx starts at 0.

    ``coord_map``: [(model coordinate, IK column, sign)]; None = every model
    coordinate from the IK column of the same name.  Locked coordinates keep
    their default value (``Coordinate.setValue`` is a no-op when locked)."""
    header, labels, arr = read_sto(ik_mot_path)
    col = {l: i for i, l in enumerate(labels)}
    t_raw = arr[:, 0]
    coord_order = list(model.coord_order)
    if coord_map is None:
        coord_map = [(c, c, 1.0) for c in coord_order]
    q = np.zeros((arr.shape[0], len(coord_order)))
    for c in coord_order:
        q[:, coord_order.index(c)] = model.coords[c].default_value
    for cm, cik, sign in coord_map:
        if model.coords[cm].locked:
            continue
        v = arr[:, col[cik]]
        if cik not in ('pelvis_tx', 'pelvis_ty', 'pelvis_tz'):
            v = v * math.pi / 180.0
        q[:, coord_order.index(cm)] = sign * v
    t, q = resample_linear(t_raw, q, dt)
    q = _lowpass(q, dt)
    for c in coord_order:
        if model.coords[c].locked:
            q[:, coord_order.index(c)] = model.coords[c].default_value
    ity = coord_order.index('pelvis_ty')
    lows = np.array([lowest_sphere_y(model, dict(zip(coord_order, row))) for row in q])
    q[:, ity] += -penetration - lows.min()
    itx = coord_order.index('pelvis_tx')
    q[:, itx] -= q[0, itx]
    u = _spline_derivative(t, q)
    for c in coord_order:
        if model.coords[c].locked:
            u[:, coord_order.index(c)] = 0.0
    bodies, com, rot = body_com_table(model, coord_order, q)
    vel = _spline_derivative(t, com)
    os.makedirs(out_dir, exist_ok=True)
    write_sto(os.path.join(out_dir, 'task_Kinematics_q.sto'), ['time'] + coord_order,
              np.column_stack([t, q]), name='Coordinates')
    write_sto(os.path.join(out_dir, 'task_Kinematics_u.sto'), ['time'] + coord_order,
              np.column_stack([t, u]), name='Speeds')
    for fname, tab in (('task_BodyKinematics_pos_global.sto', com), ('task_BodyKinematics_vel_global.sto', vel)):
        labs, cols = ['time'], [t]
        for k, b in enumerate(bodies):
            for a, ax in enumerate('XYZ'):
                labs.append(f'{b}_{ax}')
                cols.append(tab[:, k, a])
            for a, ax in enumerate(('Ox', 'Oy', 'Oz')):
                labs.append(f'{b}_{ax}')
                cols.append(rot[:, k, a] if fname.endswith('pos_global.sto') else _spline_derivative(t, rot[:, k, a]))
        for a, ax in enumerate('XYZ'):
            labs.append(f'center_of_mass_{ax}')
            cols.append(tab[:, -1, a])
        write_sto(os.path.join(out_dir, fname), labs, np.column_stack(cols), name='BodyKinematics')
    return t, q, u


def synthesize_2d_walking(model, ik_mot_path, out_dir, penetration=0.01, dt=0.01):
    """2D walking from the sagittal columns of the 3D IK (the 2D recipe's input
    ``healthy_gait.sto`` is absent)."""
    return synthesize_reference(model, ik_mot_path, out_dir, SAGITTAL_MAP_2D, penetration, dt)


def load_reference_tables(ref_dir, coord_order, dt=0.01):
    """Read the four tables the env reads (read_from_storage semantics) and
    return arrays in pack order: time, q/u (CoordinateSet order), x (REF_BODIES order)."""
    from .storage import read_from_storage
    qd = read_from_storage(os.path.join(ref_dir, 'task_Kinematics_q.sto'), dt)
    ud = read_from_storage(os.path.join(ref_dir, 'task_Kinematics_u.sto'), dt)
    xd = read_from_storage(os.path.join(ref_dir, 'task_BodyKinematics_pos_global.sto'), dt)
    n = min(len(qd), len(ud), len(xd))
    q = np.stack([qd[c].to_numpy()[:n] for c in coord_order], axis=1)
    u = np.stack([ud[c].to_numpy()[:n] for c in coord_order], axis=1)
    x = np.zeros((n, len(REF_BODIES), 3))
    for k, b in enumerate(REF_BODIES):
        for a, ax in enumerate('XYZ'):
            x[:, k, a] = xd[f'{b}_{ax}'].to_numpy()[:n]
    return dict(time=qd['time'].to_numpy()[:n], q=q, u=u, x=x)


# ------------------------------------------------- run-time reference motions
MAX_ROWS_TEXT = 'a clip may be 3 to {hi} rows after resampling at {dt} s: {lo_s:.2f} s to {hi_s:.2f} s'


class ReferenceMotion:
    """A reference motion in the form the packs carry: ``time`` [rows] (a
    0.01 s grid from 0), ``q`` / ``u`` [rows][ncoord] in CoordinateSet order
    (radians and metres), ``x`` [rows][len(REF_BODIES)][3] the mass centres of
    REF_BODIES in ground.  ``config={'reference': ref}`` gives it to an env
    (``registry.load_pack``).  ``kinematics``: the body kinematics the tables
    were made from ({'bodies', 'com', 'orient', 'system'} as arrays), which
    ``save`` writes in full."""

    def __init__(self, env_id, time, q, u, x, coords, kinematics=None):
        self.env_id, self.coords = env_id, list(coords)
        self.time, self.q, self.u, self.x = (np.asarray(a, dtype=np.float64) for a in (time, q, u, x))
        self.kinematics = kinematics

    def save(self, path):
        """The four storages the envs read, into the directory ``path``:
        ``task_Kinematics_{q,u}.sto`` and
        ``task_BodyKinematics_{pos,vel}_global.sto`` (with the kinematics the
        tables were made from: every body's columns, and ``_acc_`` too; without
        them: the REF_BODIES position columns only, and no velocity file)."""
        os.makedirs(path, exist_ok=True)
        write_sto(os.path.join(path, 'task_Kinematics_q.sto'), ['time'] + self.coords,
                  np.column_stack([self.time, self.q]), name='Coordinates')
        write_sto(os.path.join(path, 'task_Kinematics_u.sto'), ['time'] + self.coords,
                  np.column_stack([self.time, self.u]), name='Speeds')
        if self.kinematics is not None:
            from .body_kinematics import write_sto as write_bk
            write_bk(path, self.time, self.kinematics, bodies=self.kinematics['bodies'], local=False)
        else:
            labs = ['time'] + [f'{b}_{ax}' for b in REF_BODIES for ax in 'XYZ']
            write_sto(os.path.join(path, 'task_BodyKinematics_pos_global.sto'), labs,
                      np.column_stack([self.time, self.x.reshape(self.x.shape[0], -1)]), name='BodyKinematics')
        return path


def sphere_points(pk, bodies):
    """The pack's contact spheres as ``BodyKinematics`` points, [(OpenSim body
    name, centre in that body's frame)], and their radii."""
    pts, radii = [], []
    for s in range(pk.nsphere):
        sp = pk.sphere[s]
        ob = pk.osbody[sp.obody]
        R, p = np.array(ob.R).reshape(3, 3), np.array(ob.p)
        pts.append((bodies[sp.obody], tuple(R.T @ (np.array(sp.loc) - p))))
        radii.append(float(sp.radius))
    return pts, np.array(radii)


def deepest_penetration(bk, pk, q_dof):
    """max over the rows and the pack's contact spheres of radius - centre
    height: how far the lowest sphere reaches below the ground plane (one
    ``BodyKinematics.eval`` launch with the spheres as points)."""
    pts, radii = sphere_points(pk, bk.bodies)
    y = bk.eval(q_dof, points=pts, want=('point',))['point'][:, :, 0, 1].cpu().numpy()
    return float((radii[None, :] - y).max())


def reference_from_coordinates(env_id, time, q, lowpass_hz=6.0, penetration=0.01, rebase_tx=True, device=0):
    """``synthesize_reference``'s recipe from coordinates alone, without the
    ``.osim``: a ``ReferenceMotion`` for ``env_id`` from ``q`` [rows][ncoord]
    (the pack's coordinate order, radians and metres: what
    ``InverseKinematics.solve_trc`` returns) sampled at ``time`` [rows].

    Resampled linearly at 0.01 s (the grid then starts at 0: an env reads row
    ``istep``); the zero-phase Butterworth low-pass at ``lowpass_hz`` (None: no
    filter); locked coordinates held at the pack's default value, speed 0;
    pelvis_ty shifted so that the deepest contact-sphere penetration over the
    clip is ``penetration`` (None: no shift) and, with ``rebase_tx``, pelvis_tx
    starting at 0; u from the cubic-spline derivative.  The spheres' heights and
    the bodies' mass centres (``x``) come from ``BodyKinematics`` on ``device``:
    one launch each over all rows."""
    from .body_kinematics import BodyKinematics
    from .obslayout import load_names
    from .packdef import MAX_REFROWS
    from .registry import load_pack
    pk, dt = load_pack(env_id), 0.01
    coords = list(load_names(env_id)['coords'])
    time, q = np.asarray(time, dtype=np.float64), np.asarray(q, dtype=np.float64)
    if time.ndim != 1 or q.ndim != 2 or q.shape != (time.size, pk.ncoord):
        raise ValueError(f'reference_from_coordinates: time must have shape (rows,) and q (rows, {pk.ncoord}) in the '
                         f'order {coords}; got {time.shape} and {q.shape}')
    if time.size < 2 or not np.all(np.isfinite(time)) or not np.all(np.diff(time) > 0):
        raise ValueError('reference_from_coordinates: time must be finite and strictly increasing (two rows or more)')
    if not np.all(np.isfinite(q)):
        raise ValueError('reference_from_coordinates: q has non-finite entries')
    t, q = resample_linear(time, q, dt)
    if not 3 <= t.size <= MAX_REFROWS:
        raise ValueError(f'reference_from_coordinates: {t.size} rows; ' + MAX_ROWS_TEXT.format(
            hi=MAX_REFROWS, dt=dt, lo_s=2 * dt, hi_s=(MAX_REFROWS - 1) * dt))
    t = dt * np.arange(t.size, dtype=np.float64)
    if lowpass_hz is not None:
        q = _lowpass(q, dt, float(lowpass_hz))
    locked = [c for c in range(pk.ncoord) if pk.coord[c].dof < 0]
    free = [c for c in range(pk.ncoord) if pk.coord[c].dof >= 0]
    dof_of = [int(pk.coord[c].dof) for c in free]
    for c in locked:
        q[:, c] = pk.coord[c].default_value

    def dofs(a):
        out = np.zeros((a.shape[0], pk.ndof))
        out[:, dof_of] = a[:, free]
        return out
    bk = BodyKinematics(env_id, device=device)
    try:
        if penetration is not None:
            if pk.coord_ty < 0 or pk.nsphere == 0:
                raise ValueError(f'reference_from_coordinates: {env_id} has no pelvis_ty or no contact spheres to '
                                 'calibrate the ground with; pass penetration=None')
            q[:, pk.coord_ty] += deepest_penetration(bk, pk, dofs(q)) - float(penetration)
        if rebase_tx and pk.coord_tx >= 0:
            q[:, pk.coord_tx] -= q[0, pk.coord_tx]
        u = _spline_derivative(t, q)
        for c in locked:
            u[:, c] = 0.0
        out = bk.eval(dofs(q), dofs(u), dofs(_spline_derivative(t, u)), want=('com', 'orient', 'system'))
        kin = {k: v.cpu().numpy() for k, v in out.items()}
        kin['bodies'] = list(bk.bodies)
    finally:
        bk.close()
    x = np.zeros((t.size, len(REF_BODIES), 3))
    for k in range(len(REF_BODIES)):
        b = int(pk.rw_body[k])
        x[:, k] = kin['com'][:, b, 0, :] if b >= 0 else kin['system'][:, 0, :]
    return ReferenceMotion(env_id, t, q, u, x, coords, kinematics=kin)


def reference_tables(ref, coords, dt=0.01):
    """``config['reference']`` as a dict of arrays time, q, u, x: a
    ``ReferenceMotion``, a dict with those keys, or a directory holding the
    four storages (read with ``load_reference_tables`` and the pack's
    coordinate names ``coords``)."""
    if isinstance(ref, (str, os.PathLike)):
        if not os.path.isdir(ref):
            raise ValueError(f"config['reference']: {os.fspath(ref)!r} is not a directory (it must hold "
                             'task_Kinematics_{q,u}.sto and task_BodyKinematics_pos_global.sto)')
        return load_reference_tables(os.fspath(ref), list(coords), dt)
    if isinstance(ref, dict):
        missing = [k for k in ('time', 'q', 'u', 'x') if k not in ref]
        if missing:
            raise ValueError(f"config['reference']: the dict lacks {missing} (it needs time, q, u, x)")
        return {k: ref[k] for k in ('time', 'q', 'u', 'x')}
    if all(hasattr(ref, k) for k in ('time', 'q', 'u', 'x')):
        return dict(time=ref.time, q=ref.q, u=ref.u, x=ref.x)
    raise ValueError("config['reference'] must be a ReferenceMotion, a dict with time, q, u, x, or a directory with "
                     f'the four reference storages; got {type(ref).__name__}')
