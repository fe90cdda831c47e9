"""A stretch-reflex tracking drive for the muscle envs, on the device.

A ready-made excitation policy.  Per muscle a stretch reflex toward the
reference motion:

    e = clip(a0 + kl (L − L* − dL/dq · dq) / l_opt + kv (L̇ − L̇*) / l_opt, 0, 1)

L, L̇ and dL/dq are the muscle's path length, lengthening speed and moment arms
at the env's state.  L* and L̇* are those of the reference row
``min(istep + 1, nrows − 1)``, the row the observation's target block shows.
The floating base is not actuated by muscles, so the trunk is balanced
through the hips: the targets' hip flexions move by
``kb (tilt − tilt*) + kbd (tilt' − tilt'*)`` (pelvis tilt error), entered
through the linearization L* + dL/dq · dq.  Spatial models balance the pelvis
list through the hip adductions the same way (gains ``kl_b``, ``kld_b``).

The reference tables come from one ``MuscleAnalysis.eval`` launch at
construction.  A call is one ``VectorEnv.muscle_analysis`` launch at the
envs' current state plus torch arithmetic on the env's stream: no host data,
no synchronization.  With the default gains MuscleWalkingImitation2D-v0 stays
up for 200 steps (2 s) from 16 of the reset rows 0..64 (tests/tracking.py has
the CPU form of this drive and the rows).
"""
from __future__ import annotations

import numpy as np

GAINS = dict(a0=0.03, kl=20.0, kv=0.5, kb=-1.0, kbd=-0.05, kl_b=0.0, kld_b=0.0)
# the joints an ``offset`` column moves, in column order
OFFSET_COORDS = ('hip_flexion_r', 'hip_flexion_l', 'hip_adduction_r', 'hip_adduction_l',
                 'knee_angle_r', 'knee_angle_l', 'ankle_angle_r', 'ankle_angle_l')


class ReflexDrive:
    def __init__(self, venv, gains=None):
        import torch
        from .muscle_analysis import MuscleAnalysis
        from .obslayout import load_names
        from .packdef import state_row_slices
        pk = venv.pack
        if pk.nmuscle == 0:
            raise ValueError(f'ReflexDrive drives muscles; {venv.env_id} is a torque env')
        self.venv = venv
        self.g = dict(GAINS, **(gains or {}))
        nd, nm = pk.ndof, pk.nmuscle
        self.nrows = pk.nrows
        dof = {n: pk.coord[c].dof for c, n in enumerate(load_names(venv.env_id)['coords'])}
        hips = [dof['hip_flexion_r'], dof['hip_flexion_l']]
        self.tilt = dof['pelvis_tilt']
        # spatial models: the pelvis list is balanced through the hip adductions
        adds = [dof[n] for n in ('hip_adduction_r', 'hip_adduction_l') if dof.get(n, -1) >= 0]
        self.list = dof.get('pelvis_list', -1) if adds else -1
        odofs = [dof.get(n, -1) for n in OFFSET_COORDS]   # absent or locked joints: -1, skipped
        # dq = bal * hip_mask + lb * add_mask + offset @ off_map, all on the device
        hip_mask, add_mask, off_map = np.zeros(nd), np.zeros(nd), np.zeros((len(odofs), nd))
        hip_mask[hips] = 1.0
        add_mask[adds] = 1.0
        for k, d in enumerate(odofs):
            if d >= 0:
                off_map[k, d] = 1.0
        self.slices, _ = state_row_slices(nd, nm, pk.nact, pk.horizon)
        qref, uref = np.zeros((pk.nrows, nd)), np.zeros((pk.nrows, nd))
        for c in range(pk.ncoord):
            d = pk.coord[c].dof
            if d >= 0:
                qref[:, d] = [pk.ref_q[r][c] for r in range(pk.nrows)]
                uref[:, d] = [pk.ref_u[r][c] for r in range(pk.nrows)]
        dev = dict(device=venv.device, dtype=venv.dtype)
        self.qref, self.uref = torch.as_tensor(qref, **dev), torch.as_tensor(uref, **dev)
        ma = MuscleAnalysis(venv.env_id, device=venv.device.index, precision=venv.precision)
        ref = ma.eval(self.qref, self.uref, want=('length', 'speed'))
        self.Lref, self.Ldref = ref['length'], ref['speed']
        torch.cuda.synchronize(venv.device)   # the tables are complete before their env goes
        ma.close()
        self.hip_mask, self.add_mask, self.off_map = (torch.as_tensor(x, **dev) for x in (hip_mask, add_mask, off_map))
        self.lopt = torch.as_tensor([pk.muscle[m].lopt for m in range(nm)], **dev)

    def __call__(self, offset=None):
        """(N, nmuscle) excitations for ``venv``'s current state, in its dtype
        on its device.  ``offset``: (N, ≤8) joint-target offsets (radians) on
        top of the balance terms, columns as ``OFFSET_COORDS``."""
        import torch
        g, v, sl = self.g, self.venv, self.slices
        rows = v.state_rows()
        ma = v.muscle_analysis(want=('length', 'speed', 'dldq'), rows=rows)
        q, u = rows[:, sl['q']].to(v.dtype), rows[:, sl['u']].to(v.dtype)
        r = (rows[:, sl['istep'].start].long() + 1).clamp(max=self.nrows - 1)
        qr, ur = self.qref[r], self.uref[r]
        t = self.tilt
        bal = g['kb'] * (q[:, t] - qr[:, t]) + g['kbd'] * (u[:, t] - ur[:, t])
        dq = bal[:, None] * self.hip_mask
        if self.list >= 0:
            ls = self.list
            lb = g['kl_b'] * (q[:, ls] - qr[:, ls]) + g['kld_b'] * (u[:, ls] - ur[:, ls])
            dq = dq + lb[:, None] * self.add_mask
        if offset is not None:
            off = torch.as_tensor(offset, device=v.device, dtype=v.dtype)
            if off.dim() != 2 or off.shape[0] != v.num_envs or off.shape[1] > self.off_map.shape[0]:
                raise ValueError(f'offset must have shape ({v.num_envs}, <= {self.off_map.shape[0]}), '
                                 f'got {tuple(off.shape)}')
            dq = dq + off @ self.off_map[:off.shape[1]]
        lin = (ma['dldq'] * dq[:, None, :]).sum(-1)
        e = g['a0'] + g['kl'] * (ma['length'] - self.Lref[r] - lin) / self.lopt + \
            g['kv'] * (ma['speed'] - self.Ldref[r]) / self.lopt
        return e.clamp_(0.0, 1.0)
