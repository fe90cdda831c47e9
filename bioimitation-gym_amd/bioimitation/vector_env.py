"""Batched env over the HIP C-ABI: N environments of one registered ID on
one GPU, stepped by one kernel launch.

This is the throughput surface (RLlib ``VectorEnv`` / gym vector-env shaped);
:class:`bioimitation.envs.ImitationEnv` is the single-instance, reference-
shaped surface built on top of it.  Buffers are torch tensors on the GPU;
each launch runs on torch's *current* stream of that device at the time of
the call (the handle is re-bound when the caller switches streams), so it
orders with the caller's torch work.

Aliasing: ``reset()`` and ``step()`` return the env's persistent output
tensors (``self.obs``, ``self.reward``, ``self.done``, ``self.info``), which
the next launch overwrites in place — zero-copy for callers that consume a
step before issuing the next.  Keep a result across steps with ``.clone()``
(the adapters in :mod:`bioimitation.adapters` do).  With auto-reset on, a
done env's row holds its post-reset observation; ``enable_final_obs()``
keeps the terminal one in ``self.final_obs``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .registry import load_pack

INTEGRATORS = {'semi-implicit': 0, 'rk-merson': 1}
OSIM_OPS = {'realize': 0, 'equilibrate': 1, 'integrate': 2}   # include/bioim.h BIOIM_OSIM_*


def check_env_mask(mask, num_envs, device):
    """A per-env mask the step kernel may read: a contiguous (num_envs,)
    uint8/bool tensor on the env's device (or None).  Anything else would
    make the kernel read host memory or past the end of the buffer."""
    import torch
    if mask is None:
        return
    if not isinstance(mask, torch.Tensor):
        raise ValueError('env mask must be a torch tensor (or None)')
    if mask.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f'env mask dtype must be uint8 or bool, got {mask.dtype}')
    if mask.device != torch.device(device):
        raise ValueError(f'env mask must be on {device}, got {mask.device}')
    if mask.dim() != 1 or mask.numel() != num_envs:
        raise ValueError(f'env mask must have shape ({num_envs},), got {tuple(mask.shape)}')
    if not mask.is_contiguous():
        raise ValueError('env mask must be contiguous')


def _rollout_buffers(env, actions, steps, obs, info, stop_with_auto_reset, out, zero):
    """``rollout()``'s argument checks for a batch ``env`` (its num_envs,
    action_dim, obs_dim, info_dim, dtype and device): the actions as the
    kernel reads them, T, the action stride between steps in elements, and
    the sequence buffers by name — the caller's ``out`` entries, checked, or
    new tensors (zero-filled with ``zero``)."""
    import torch
    if obs not in ('last', 'all', None):
        raise ValueError(f"rollout: obs must be 'last', 'all' or None, got {obs!r}")
    if not isinstance(actions, torch.Tensor):
        raise ValueError('rollout: actions must be a torch tensor')
    n, na = env.num_envs, env.action_dim
    if actions.dim() == 2:
        if steps is None:
            raise ValueError('rollout: (N, A) actions need steps=T')
        T, stride = int(steps), 0
        want = (n, na)
    else:
        T = int(actions.shape[0]) if actions.dim() == 3 else 0
        if steps is not None and int(steps) != T:
            raise ValueError(f'rollout: steps={steps} but actions hold {T} steps')
        stride = n * na
        want = (T, n, na)
    if T <= 0 or tuple(actions.shape) != want:
        raise ValueError(f'rollout: actions must have shape (T, {n}, {na}) or ({n}, {na}) with steps=T >= 1, '
                         f'got {tuple(actions.shape)}')
    if stop_with_auto_reset:
        raise ValueError('rollout: stop_at_done needs auto-reset off')
    a = actions
    if a.dtype != env.dtype or a.device != env.device or not a.is_contiguous():
        a = a.to(device=env.device, dtype=env.dtype).contiguous()
    out = dict(out or {})
    unknown = set(out) - {'obs', 'reward', 'done', 'info'}
    if unknown:
        raise ValueError(f'rollout: unknown out buffers {sorted(unknown)}')
    shapes = {'reward': ((T, n), env.dtype), 'done': ((T, n), torch.uint8)}
    if obs == 'all':
        shapes['obs'] = ((T, n, env.obs_dim), env.dtype)
    if info:
        shapes['info'] = ((T, n, env.info_dim), env.dtype)
    for k in out:
        if k not in shapes:
            raise ValueError(f"rollout: out['{k}'] given but not asked for (obs={obs!r}, info={info})")
    buf = {}
    for k, (shape, dtype) in shapes.items():
        if k in out:
            buf[k] = VectorEnv._check_seq(env, out[k], shape, dtype, f"out['{k}']")
        else:
            buf[k] = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=env.device)
    return a, T, stride, buf


class VectorEnv:
    def __init__(self, env_id: str, num_envs: int, config: dict = None, device: int = 0, precision: int = 64,
                 seed: int = 0, auto_reset: bool = False, env_offset: int = 0):
        import torch
        if not torch.cuda.is_available():
            raise _lib.BioimError('VectorEnv needs a HIP GPU (no CPU fallback)')
        L = _lib.load()
        self.env_id = env_id
        self.config = dict(config or {})
        self.pack = load_pack(env_id, config)
        self.num_envs = int(num_envs)
        self.device = torch.device('cuda', device)
        self.precision = precision
        self.dtype = torch.float32 if precision == 32 else torch.float64
        h = C.c_void_p()
        _lib.check(L.bioim_create(C.byref(self.pack), self.num_envs, device, precision, seed, C.byref(h)))
        self._h = h
        self._L = L
        self._stream = None
        self._bind_stream()
        q = (C.c_int32 * 8)()
        _lib.check(L.bioim_query(h, q))
        self.obs_dim, self.action_dim, self.info_dim, self.lanes_per_env, self.nsub, self.state_dim = \
            q[1], q[2], q[3], q[5], q[6], q[7]
        ql = (C.c_int32 * 5)()
        _lib.check(L.bioim_query_launch(h, ql))
        self.launch = dict(lanes_per_env=ql[0], threads_per_workgroup=ql[1], envs_per_workgroup=ql[2],
                           lds_bytes_per_workgroup=ql[3], workgroups=ql[4])
        _lib.check(L.bioim_set_auto_reset(h, 1 if auto_reset else 0))
        self._auto_reset = bool(auto_reset)
        # config 'integrator': 'semi-implicit' (fixed substeps, the default) or 'rk-merson' (the
        # reference's adaptive integrator at 'integrator_accuracy', default the env's 1e-3)
        self.integrator = (config or {}).get('integrator', 'semi-implicit')
        if self.integrator not in INTEGRATORS:
            raise ValueError(f"integrator must be one of {sorted(INTEGRATORS)}, got {self.integrator!r}")
        self.integrator_accuracy = float((config or {}).get('integrator_accuracy', 1e-3))
        _lib.check(L.bioim_set_integrator(h, INTEGRATORS[self.integrator], self.integrator_accuracy))
        _lib.check(L.bioim_set_env_offset(h, int(env_offset)))
        self.env_offset = int(env_offset)
        n = self.num_envs
        self.obs = torch.zeros((n, self.obs_dim), dtype=self.dtype, device=self.device)
        self.reward = torch.zeros(n, dtype=self.dtype, device=self.device)
        self.done = torch.zeros(n, dtype=torch.uint8, device=self.device)
        self.info = torch.zeros((n, self.info_dim), dtype=self.dtype, device=self.device)
        self.final_obs = None
        self.perturbation = None
        self.external_forces = None     # set_external_forces: (body names, frame names, the (N, K, 9) tensor)
        if (config or {}).get('apply_perturbations'):
            from .perturb import batch_points
            self.set_perturbation(*batch_points(env_id, n, seed=(config or {}).get('perturbation_seed', seed),
                                                env_offset=env_offset))

    def set_perturbation(self, x, y, body='torso'):
        """apply_perturbations (muscle_walking_imitation_env2D.py:83-100): the
        reference's PiecewiseConstantFunction points ``x`` [n] (shared) and
        ``y`` [num_envs][n] (N) of the ground-x force on ``body``'s origin;
        ``x=None`` removes it.  Converted to the device's zero-order-hold
        table by :func:`bioimitation.perturb.zoh_table`."""
        from .obslayout import load_names
        from .perturb import os_body_index, zoh_table
        if x is not None and self.external_forces is not None:
            raise ValueError('set_perturbation: external forces are set on this env (set_external_forces); a push '
                             'is one force slot there')
        if x is None:
            _lib.check(self._L.bioim_set_perturbation(self._h, -1, 0, None, None))
            self.perturbation = None
            return
        xt, yt = zoh_table(x, y)
        yt = np.ascontiguousarray(np.broadcast_to(yt, (self.num_envs, len(xt))), dtype=np.float64)
        ob = os_body_index(load_names(self.env_id), body)
        dp = C.POINTER(C.c_double)
        xt = np.ascontiguousarray(xt)
        _lib.check(self._L.bioim_set_perturbation(self._h, ob, len(xt), xt.ctypes.data_as(dp), yt.ctypes.data_as(dp)))
        self.perturbation = (np.asarray(x, dtype=np.float64), yt)

    def set_external_forces(self, points, wrench=None, point_in='body'):
        """Per-env external forces and torques on bodies
        (``bioimitation.external_forces``; ``bioim_set_external_forces``).
        ``points``: up to 8 OpenSim body names, one per force slot (a body may
        have several); ``point_in``: 'body' or 'ground', one for all or one
        per slot — the frame the slot's point of application is given in.
        ``wrench``: a contiguous (N, K, 9) tensor of the env's dtype on its
        device, per env and slot ``fx fy fz px py pz tx ty tz`` (force and
        torque in ground); None allocates zeros.  Returns the tensor every
        later ``step``, ``reset``, ``osim`` call and rollout step reads at its
        start: write into it between steps on the env's stream, like actions.
        The values are held over a step; they are inputs, not state
        (``state_rows`` / ``load_state`` / ``clone_envs`` leave them alone, an
        auto-reset too) and are not sanitized.  ``points=None`` removes the
        forces.  Not with ``apply_perturbations`` or ``integrator='rk-merson'``
        (``ValueError``); a rollout then runs one launch per step."""
        import torch
        from . import external_forces as xf
        if points is None:
            self._bind_stream()
            _lib.check(self._L.bioim_set_external_forces(self._h, 0, None, None, None))
            self.external_forces = None
            return None
        if getattr(self, '_bk_bodies', None) is None:
            from .obslayout import load_names
            self._bk_bodies = list(load_names(self.env_id)['bodies'])
        body, frame = xf.check_slots(self._bk_bodies, points, point_in)
        xf.check_compatible(self.perturbation, self.integrator, getattr(self, 'rk_budget', 0))
        k = int(body.size)
        if wrench is None:
            wrench = torch.zeros((self.num_envs, k, xf.ROW), dtype=self.dtype, device=self.device)
        xf.check_wrench(wrench, self.num_envs, k, self.dtype, self.device)
        ip = C.POINTER(C.c_int32)
        self._bind_stream()
        _lib.check(self._L.bioim_set_external_forces(self._h, k, body.ctypes.data_as(ip), frame.ctypes.data_as(ip),
                                                     self._ptr(wrench)))
        self.external_forces = (body, frame, wrench)
        return wrench

    def external_wrench_ground(self, env_ids=None, rows=None):
        """The current external forces as the analyses take them (``ext`` of
        ``joint_reaction`` / ``induced_accelerations``): ``[n][ncbody][6]``,
        fx fy fz mx my mz on each composite body in the ground frame, the
        moment about the ground origin; one row per env (or per listed env, in
        the list's order).  Formed on the device from the envs' own
        ``body_kinematics`` origins and rotations and the (N, K, 9) tensor as
        it is now: no host round trip, no synchronization.  None when no
        forces are set."""
        import torch
        from . import external_forces as xf
        if self.external_forces is None:
            return None
        body, frame, wrench = self.external_forces
        pk = self.pack
        if env_ids is not None:
            host, ids = self._id_list(env_ids, 'env', distinct=True)
            if ids is None:
                ids = self._upload_ids(host)
            wrench = wrench.index_select(0, ids.long())
        bk = self.body_kinematics(env_ids=env_ids, want=('origin', 'rot'), rows=rows)
        cbody = [pk.osbody[b].cbody for b in range(pk.nosbody)]
        return xf.wrench_ground(wrench, body, frame, cbody, pk.ncbody, bk['origin'][:, :, 0, :], bk['rot'])

    def set_reset_table(self, on: bool = True):
        """In-kernel auto-resets from the per-handle reset table (default on;
        bioim_set_reset_table): muscle models with the default step kernels
        read the drawn row's reset state and observation instead of running
        the reset realize in the step launch."""
        _lib.check(self._L.bioim_set_reset_table(self._h, 1 if on else 0))

    @property
    def reset_table_rows(self) -> int:
        """rows of the built reset table (0: not built / not used)"""
        return _lib.check(self._L.bioim_reset_table_rows(self._h))

    def _bind_stream(self):
        """Launch on torch's current stream of the env's device (re-bound
        whenever the caller has switched streams since the last launch)."""
        import torch
        s = torch.cuda.current_stream(self.device).cuda_stream
        if s != self._stream:
            _lib.check(self._L.bioim_set_stream(self._h, C.c_void_p(s)))
            self._stream = s

    def enable_final_obs(self, on: bool = True):
        """Keep each step's observation from before an in-kernel auto-reset in
        ``self.final_obs`` (N, O): a done env's terminal observation (gym's
        ``final_observation``); equal to ``obs`` for envs that did not reset."""
        import torch
        if on and self.final_obs is None:
            self.final_obs = torch.zeros_like(self.obs)
        elif not on:
            self.final_obs = None
        _lib.check(self._L.bioim_set_final_obs(self._h, self._ptr(self.final_obs)))

    @property
    def force_report_dim(self) -> int:
        """F of the force-report rows (bioim_force_report_dim)"""
        return _lib.check(self._L.bioim_force_report_dim(self._h))

    def enable_force_report(self, on: bool = True, out=None):
        """Per-force-element values of every realized state in
        ``self.force_report`` (N, F), F = bioim_force_report_dim (include/bioim.h);
        ``out``: a contiguous (N, F) tensor of the env's dtype and device to
        write them to instead (e.g. a view of a larger buffer)."""
        import torch
        if on and out is not None:
            f = self.force_report_dim
            if out.shape != (self.num_envs, f) or out.dtype != self.dtype or out.device != self.device \
                    or not out.is_contiguous():
                raise ValueError(f'force report buffer must be a contiguous ({self.num_envs}, {f}) {self.dtype} '
                                 f'tensor on {self.device}')
            self.force_report = out
        elif on and getattr(self, 'force_report', None) is None:
            f = _lib.check(self._L.bioim_force_report_dim(self._h))
            self.force_report = torch.zeros((self.num_envs, f), dtype=self.dtype, device=self.device)
        elif not on:
            self.force_report = None
        _lib.check(self._L.bioim_set_force_report(self._h, self._ptr(self.force_report)))

    def enable_state_storage(self, capacity: int = 64):
        """RK integrator: the state at every accepted integration step of each
        env step in ``self.storage_rows`` (N, capacity, 1 + 2 ndof + 2 nm: t,
        q, u, activation, fiber length) and their number in
        ``self.storage_count`` (bioim_set_state_storage).  ``capacity=0`` turns
        it off."""
        import torch
        if capacity:
            d = 1 + 2 * self.pack.ndof + 2 * self.pack.nmuscle
            self.storage_rows = torch.zeros((self.num_envs, capacity, d), dtype=self.dtype, device=self.device)
            self.storage_count = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        else:
            self.storage_rows = self.storage_count = None
        _lib.check(self._L.bioim_set_state_storage(self._h, self._ptr(self.storage_rows), int(capacity),
                                                   self._ptr(self.storage_count)))
        self._storage_grow = 0

    def grow_state_storage(self, capacity: int):
        """Ask for at least ``capacity`` storage rows from the NEXT ``step()``
        on: the reallocation (which zeroes ``storage_rows`` / ``storage_count``
        for every env of the batch) is deferred to just before that step's
        launch, so every reader of the current step's rows still sees them."""
        self._storage_grow = max(getattr(self, '_storage_grow', 0), int(capacity))

    def _apply_storage_growth(self):
        k = getattr(self, '_storage_grow', 0)
        if k and getattr(self, 'storage_rows', None) is not None and k > self.storage_rows.shape[1]:
            self.enable_state_storage(k)
        self._storage_grow = 0

    def set_rk_budget(self, attempts: int):
        """Budgeted steps for the 'rk-merson' integrator (``bioim_set_rk_budget``):
        each ``step()`` gives every env at most ``attempts`` Kutta-Merson step
        attempts; an env not finished by then resumes in the next ``step()``
        (its action row is ignored until then) and is 0 in ``self.ready``.
        Only ready rows of obs / reward / done / info are fresh.  The
        trajectories equal the unbudgeted run's bit for bit; a launch is no
        longer as long as its stiffest env.  ``attempts=0`` turns it off."""
        import torch
        if self.integrator != 'rk-merson' and attempts:
            raise ValueError("set_rk_budget needs config integrator='rk-merson'")
        if attempts and self.external_forces is not None:
            raise ValueError('set_rk_budget: external forces are set on this env (set_external_forces): '
                             'semi-implicit only')
        self.rk_budget = int(attempts)
        if attempts and getattr(self, 'ready', None) is None:
            self.ready = torch.ones(self.num_envs, dtype=torch.uint8, device=self.device)
        elif not attempts:
            self.ready = None
        _lib.check(self._L.bioim_set_rk_budget(self._h, self.rk_budget, self._ptr(self.ready)))

    def set_active_mask(self, mask):
        """Per-env step mask (``bioim_set_active_mask``): a (N,) uint8 device
        tensor read by every later ``step()``; envs with 0 are left untouched
        unless they are finishing a suspended RK step.  ``None`` steps all.
        The tensor must stay alive while it is set."""
        check_env_mask(mask, self.num_envs, self.device)
        self._active = mask
        _lib.check(self._L.bioim_set_active_mask(self._h, self._ptr(mask)))

    def osim(self, op, env_ids, controls=None, want_obs=True):
        """OsimModel calls on the listed envs (``bioim_osim``): optional
        ``controls`` (n, nact) actuated first (NaN -> 0, clip, held), then op
        'realize' (nothing else), 'equilibrate' (reset_manager: a new integrator
        and the muscles' static fiber equilibrium at the held state) or
        'integrate' (istep += 1, integrate to step_size * istep), then the
        realize.  Returns the report rows (N, bioim_osim_report_dim) — rows of
        the listed envs are fresh — and writes their obs rows into
        ``self.obs`` when ``want_obs``."""
        import torch
        if getattr(self, 'osim_report', None) is None:
            d = _lib.check(self._L.bioim_osim_report_dim(self._h))
            self.osim_report = torch.zeros((self.num_envs, d), dtype=self.dtype, device=self.device)
        ids = self._env_ids(env_ids)
        ctl = None
        if controls is not None:
            ctl = torch.as_tensor(controls, dtype=self.dtype, device=self.device).reshape(ids.numel(), self.action_dim)
            ctl = ctl.contiguous()
        if getattr(self, '_storage_grow', 0):
            self._apply_storage_growth()
        self._bind_stream()
        _lib.check(self._L.bioim_osim(self._h, OSIM_OPS[op], self._ptr(ids), ids.numel(), self._ptr(ctl),
                                      self._ptr(self.obs) if want_obs else None, self._ptr(self.osim_report)))
        return self.osim_report

    def _env_ids(self, env_ids):
        """validated int32 device tensor of env ids: in range (a stray id is an
        out-of-bounds store in the kernel) and distinct (two lane groups would
        race on one env's state)"""
        import torch
        ids = torch.as_tensor(env_ids, dtype=torch.int32, device=self.device).reshape(-1).contiguous()
        if ids.numel():
            h = ids.cpu()
            if int(h.min()) < 0 or int(h.max()) >= self.num_envs:
                raise ValueError(f'env ids must lie in [0, {self.num_envs})')
            if h.unique().numel() != h.numel():
                raise ValueError('env ids must be distinct')
        return ids

    @property
    def build_id(self) -> str:
        """bioim_build_id() of the loaded library (sources + flags hash)"""
        return self._L.bioim_build_id().decode()

    def pending_count(self) -> int:
        """Envs suspended mid-step by the RK budget."""
        return _lib.check(self._L.bioim_pending_count(self._h))

    @staticmethod
    def _ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def set_auto_reset(self, on: bool):
        _lib.check(self._L.bioim_set_auto_reset(self._h, 1 if on else 0))
        self._auto_reset = bool(on)

    def reset(self, env_ids=None, ref_index=None):
        """Reset the listed envs (default all).  ref_index: reference rows
        (default: randint(0, reset_hi) drawn on the device)."""
        import torch
        ids = rows = None
        n = self.num_envs
        if env_ids is not None:
            ids = self._env_ids(env_ids)
            n = ids.numel()
            if n == 0:          # nothing listed: nothing to reset (a null id list would mean every env)
                return self.obs
        if ref_index is not None:
            rows = torch.as_tensor(ref_index, dtype=torch.int32, device=self.device).contiguous()
            if ids is None:
                ids = torch.arange(self.num_envs, dtype=torch.int32, device=self.device)
            assert rows.numel() == n
        self._bind_stream()
        _lib.check(self._L.bioim_reset(self._h, self._ptr(ids), self._ptr(rows), n, self._ptr(self.obs)))
        return self.obs

    def step(self, actions):
        """actions: (N, nact) tensor on the env's device (dtype = precision)."""
        a = actions
        if a.dtype != self.dtype or a.device != self.device or not a.is_contiguous():
            a = a.to(device=self.device, dtype=self.dtype).contiguous()
        assert a.shape == (self.num_envs, self.action_dim), a.shape
        if getattr(self, '_storage_grow', 0):
            self._apply_storage_growth()
        self._bind_stream()
        _lib.check(self._L.bioim_step(self._h, self._ptr(a), self._ptr(self.obs), self._ptr(self.reward),
                                      self._ptr(self.done), self._ptr(self.info)))
        return self.obs, self.reward, self.done, self.info

    def _check_seq(self, t, shape, dtype, what):
        """a caller buffer the rollout writes prod(shape) elements through"""
        import torch
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype \
                or t.device != self.device or not t.is_contiguous():
            raise ValueError(f'rollout: {what} must be a contiguous {tuple(shape)} {dtype} tensor on {self.device}')
        return t

    def rollout(self, actions, steps=None, *, obs='last', info=False, stop_at_done=False, out=None):
        """T consecutive env steps from an action sequence, enqueued by one
        call with nothing on the host in between (``bioim_rollout``): with the
        default step configuration one kernel launch, otherwise (push table,
        'rk-merson', force report, state storage) T launches from C — see
        ``last_rollout_fused``.  Bit for bit what T ``step()`` calls give.

        ``actions``: (T, N, A), or (N, A) with ``steps=T`` to repeat one action
        block (frame skip); dtype / device / contiguity as in ``step()``.
        ``obs``: 'last' (the last step's rows, written to ``self.obs``, so a
        following ``step()`` composes as usual), 'all' ((T, N, O); ``self.obs``
        gets the last rows too) or None.  ``info``: also the (T, N, I) rows.
        ``stop_at_done`` (auto-reset off only): an env is not stepped again
        after its first done; its later rows are reward 0, done 1, info 0 and
        its terminal observation.  The active mask is honoured and left alone.
        ``out``: a dict of caller buffers to write to instead of new tensors —
        'reward' (T, N), 'done' (T, N) uint8, 'obs' (T, N, O) with obs='all',
        'info' (T, N, I); contiguous, of the env's dtype, on its device.

        Returns (obs, reward (T, N), done (T, N) uint8, info or None)."""
        a, T, stride, buf = _rollout_buffers(self, actions, steps, obs, info, stop_at_done and self._auto_reset, out,
                                             zero=False)
        obs_seq, obs_last = buf.get('obs'), (self.obs if obs is not None else None)
        if getattr(self, '_storage_grow', 0):
            self._apply_storage_growth()
        self._bind_stream()
        _lib.check(self._L.bioim_rollout(self._h, self._ptr(a), T, stride, self._ptr(obs_seq), self._ptr(obs_last),
                                         self._ptr(buf['reward']), self._ptr(buf['done']), self._ptr(buf.get('info')),
                                         1 if stop_at_done else 0))
        return (self.obs if obs == 'last' else obs_seq), buf['reward'], buf['done'], buf.get('info')

    @property
    def last_rollout_fused(self) -> bool:
        """True if the last ``rollout()`` ran as ONE launch of the rollout
        kernel, False if it looped over the step kernels (bioim_rollout_fused)."""
        return bool(_lib.check(self._L.bioim_rollout_fused(self._h)))

    def get_state(self) -> np.ndarray:
        s = np.zeros((self.num_envs, self.state_dim))
        _lib.check(self._L.bioim_get_state(self._h, s.ctypes.data_as(C.POINTER(C.c_double))))
        return s

    def _id_list(self, ids, what, distinct):
        """Env ids for the indexed state calls -> (host int64 array, int32
        device tensor or None).  Lists, ranges and numpy arrays are checked on
        the host alone (no device synchronization; ``_upload_ids`` then takes
        them to the device).  A device tensor goes through ``_env_ids`` (one
        synchronizing copy back) and is returned as the second value.  Ids
        lie in [0, num_envs) and, with ``distinct``, do not repeat."""
        import torch
        if isinstance(ids, torch.Tensor):
            if ids.dtype in (torch.bool, torch.float16, torch.bfloat16, torch.float32, torch.float64):
                raise ValueError(f'{what} ids must be integers, got {ids.dtype}')
            if distinct:
                dev = self._env_ids(ids)
                return dev.cpu().numpy().astype(np.int64), dev
            dev = torch.as_tensor(ids, dtype=torch.int32, device=self.device).reshape(-1).contiguous()
            ids = dev.cpu().numpy()
        else:
            dev = None
        host = np.asarray(ids).reshape(-1)
        if host.size and host.dtype.kind not in 'iu':
            raise ValueError(f'{what} ids must be integers, got {host.dtype}')
        host = host.astype(np.int64)
        if host.size and (host.min() < 0 or host.max() >= self.num_envs):
            raise ValueError(f'{what} ids must lie in [0, {self.num_envs})')
        if distinct and np.unique(host).size != host.size:
            raise ValueError(f'{what} ids must be distinct')
        return host, dev

    def _upload_ids(self, host):
        """host ids (any shape) as an int32 device tensor, copied from pinned
        memory on the current stream without waiting for the device"""
        import torch
        return torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32)).pin_memory().to(self.device, non_blocking=True)

    def _check_rows(self, t, n, what):
        """a buffer the state kernels read or write n * state_dim doubles of"""
        import torch
        if not isinstance(t, torch.Tensor) or t.shape != (n, self.state_dim) or t.dtype != torch.float64 \
                or t.device != self.device or not t.is_contiguous():
            raise ValueError(f'{what} must be a contiguous ({n}, {self.state_dim}) torch.float64 tensor on {self.device}')

    def state_rows(self, out=None, env_ids=None):
        """The flat state rows of get_state as a (N, state_dim) float64 device
        tensor, gathered on the env's stream without synchronizing
        (bioim_copy_state): one transfer can carry them with a step's
        outputs.  ``env_ids``: the rows of the listed envs only, in the
        list's order, as (len(env_ids), state_dim) (bioim_copy_state_rows).
        ``out``: a contiguous float64 tensor of that shape on the env's
        device to write them to."""
        import torch
        ids = None
        n = self.num_envs
        if env_ids is not None:
            host, ids = self._id_list(env_ids, 'env', distinct=False)
            n = host.size
        if out is None:
            out = torch.empty((n, self.state_dim), dtype=torch.float64, device=self.device)
        else:
            self._check_rows(out, n, 'state_rows: out')
        if n == 0:
            return out
        self._bind_stream()
        if env_ids is not None and ids is None:
            ids = self._upload_ids(host)
        if ids is None:
            _lib.check(self._L.bioim_copy_state(self._h, self._ptr(out)))
        else:
            _lib.check(self._L.bioim_copy_state_rows(self._h, self._ptr(ids), n, self._ptr(out)))
        return out

    def muscle_analysis(self, env_ids=None, want=('length', 'speed', 'dldq'), rows=None):
        """Muscle analysis (``bioimitation.muscle_analysis``) at the envs'
        current state: {key: device tensor} for the keys of ``want``, one row
        per env (or per listed env, in the list's order).  q, u, activations
        and fiber lengths are gathered on the device (``state_rows``) and go
        to one ``bioim_muscle_eval`` launch on the env's stream: no host round
        trip, no synchronization, and the envs are only read.  ``rows``: state
        rows already gathered for these envs (``state_rows``' result), to
        spare the gather."""
        from . import muscle_analysis as ma
        from .packdef import state_row_slices
        pk = self.pack
        if rows is None:
            rows = self.state_rows(env_ids=env_ids)
        sl, _ = state_row_slices(pk.ndof, pk.nmuscle, pk.nact, pk.horizon)
        q, u, act, lce = (rows[:, sl[f]].to(self.dtype).contiguous() for f in ('q', 'u', 'act', 'lce'))
        _, want = ma.check_args(pk.ndof, pk.nmuscle, q, u, act, lce, want)
        return ma.launch(self, q, u, act, lce, want)

    def static_optimization(self, qdd=None, tau=None, env_ids=None, reserve=1.0, lo=0.0, hi=1.0, passive=False,
                            want=('act',), rows=None):
        """Static optimization (``bioimitation.static_optimization``) at the
        envs' current q and u: the activations that produce the target
        generalized force at least effort, one row per env (or per listed
        env, in the list's order).  Exactly one of ``qdd`` (accelerations; the
        target is then their inverse-dynamics residual) and ``tau`` (the
        target itself), ``[rows][ndof]``.  q and u are gathered on the device
        (``state_rows``) and go to the launches on the env's stream: no host
        round trip, no synchronization, and the envs are only read.  Muscle
        envs in fp64 only (``ValueError`` otherwise).  ``rows``: state rows
        already gathered for these envs, to spare the gather."""
        from . import static_optimization as so
        from .packdef import state_row_slices
        pk = self.pack
        so.check_env(self)
        if rows is None:
            rows = self.state_rows(env_ids=env_ids)
        sl, _ = state_row_slices(pk.ndof, pk.nmuscle, pk.nact, pk.horizon)
        q, u = (rows[:, sl[f]].contiguous() for f in ('q', 'u'))
        _, want, lam = so.check_args(pk.ndof, pk.nmuscle, q, u, qdd, tau, reserve, lo, hi, want)
        return so.solve_on(self, q, u, qdd, tau, lam, lo, hi, passive, want)

    def computed_muscle_control(self, qdd=None, tau=None, env_ids=None, q1=None, window=0.01, nsub=None, reserve=1.0,
                                emin=0.0, emax=1.0, ftol=1e-6, max_iter=30, want=('excitation',), rows=None):
        """Computed muscle control (``bioimitation.computed_muscle_control``)
        at the envs' current q, u, activations and fiber lengths: the
        excitations whose muscles deliver the target generalized force at the
        end of ``window``, one row per env (or per listed env, in the list's
        order).  Exactly one of ``qdd`` (accelerations; the target is then
        their inverse-dynamics residual) and ``tau`` (the target itself),
        ``[rows][ndof]``.  The state is gathered on the device
        (``state_rows``) and goes to the launches on the env's stream: no host
        round trip, no synchronization, and the envs are only read.  Muscle
        envs in fp64 only (``ValueError`` otherwise).  ``rows``: state rows
        already gathered for these envs, to spare the gather."""
        from . import computed_muscle_control as cmc
        from .packdef import state_row_slices
        pk = self.pack
        cmc.check_env(self)
        if rows is None:
            rows = self.state_rows(env_ids=env_ids)
        sl, _ = state_row_slices(pk.ndof, pk.nmuscle, pk.nact, pk.horizon)
        q, u, act, lce = (rows[:, sl[f]].contiguous() for f in ('q', 'u', 'act', 'lce'))
        _, want, lam = cmc.check_args(pk.ndof, pk.nmuscle, q, u, act, lce, tau, qdd, q1, window, nsub, reserve,
                                      emin, emax, ftol, max_iter, want)
        return cmc.solve_on(self, q, u, act, lce, tau, qdd, q1, lam, window, nsub, emin, emax, ftol, max_iter, want)

    def _realize_report(self, ids, n):
        """The REALIZE report rows of the n listed envs (``ids``: a checked
        int32 device tensor) into ``self.osim_report``, on the env's stream.
        ``bioim_realize_report`` does it without reading anything back; a
        handle that has had an RK budget is refused there (its envs may be
        suspended mid-step) and goes through ``osim('realize')``, which reads
        the suspended-step flags back first."""
        import torch
        if getattr(self, 'osim_report', None) is None:
            d = _lib.check(self._L.bioim_osim_report_dim(self._h))
            self.osim_report = torch.zeros((self.num_envs, d), dtype=self.dtype, device=self.device)
        if getattr(self, '_storage_grow', 0):
            self._apply_storage_growth()
        self._bind_stream()
        if not getattr(self, '_realize_sync', False):
            rc = self._L.bioim_realize_report(self._h, self._ptr(ids), n, self._ptr(self.osim_report))
            if rc >= 0:
                return self.osim_report
            if b'RK budget' not in self._L.bioim_last_error():
                _lib.check(rc)
            self._realize_sync = True     # the refusal is for the handle's lifetime
        return self.osim('realize', ids, want_obs=False)

    def _own_state_inputs(self, env_ids, rows):
        """What the analyses at the envs' own state start from (``joint_reaction``,
        ``induced_accelerations``): (n, q, u, realize), with q and u from
        the state rows (gathered on the device unless ``rows`` has them) and
        ``realize()`` the REALIZE report rows of those envs, in their order,
        cut by the report's layout (include/bioim.h: time, istep, q[nc], u[nc],
        qdd[nc], 18 per OpenSim body, the COM's 9, 7 per muscle with the tendon
        force last, then one per actuator) into a dict: 'qdd' [n][ndof],
        'ft' [n][nmuscle] (None without muscles), 'act' [n][nact]."""
        import torch
        from .packdef import state_row_slices
        pk = self.pack
        host = None
        if env_ids is None:
            n, ids = self.num_envs, torch.arange(self.num_envs, dtype=torch.int32, device=self.device)
        else:
            host, ids = self._id_list(env_ids, 'env', distinct=True)
            n = host.size
        if rows is None:
            rows = self.state_rows(env_ids=env_ids)
        sl, _ = state_row_slices(pk.ndof, pk.nmuscle, pk.nact, pk.horizon)
        q, u = (rows[:, sl[f]].to(self.dtype).contiguous() for f in ('q', 'u'))

        def realize():
            dev_ids = ids if ids is not None else self._upload_ids(host)
            rep = self._realize_report(dev_ids, n).index_select(0, dev_ids.long())
            if getattr(self, '_jr_dof_coord', None) is None:
                coord_of = [c for d in range(pk.ndof) for c in range(pk.ncoord) if pk.coord[c].dof == d]
                self._jr_dof_coord = torch.as_tensor(coord_of, dtype=torch.long).to(self.device, non_blocking=True)
            k = 2 + 2 * pk.ncoord
            out = dict(qdd=rep[:, k:k + pk.ncoord].index_select(1, self._jr_dof_coord).contiguous(), ft=None)
            k = 2 + 3 * pk.ncoord + 18 * pk.nosbody + 9
            if pk.nmuscle:
                out['ft'] = rep[:, k:k + 7 * pk.nmuscle].reshape(n, pk.nmuscle, 7)[:, :, 6].contiguous()
            k += 7 * pk.nmuscle
            out['act'] = rep[:, k:k + pk.nact]
            return out
        return n, q, u, realize

    def joint_reaction(self, env_ids=None, frame='child', on='child', want=('reaction',), rows=None):
        """Joint reactions (``bioimitation.joint_reaction``) at the envs' own
        state: {key: device tensor} for the keys of ``want``, one row per env
        (or per listed env, in the list's order; distinct ids).  q and u are
        gathered on the device (``state_rows``); the accelerations and the
        muscles' tendon forces come from a REALIZE report of those envs
        (``bioim_realize_report``), which leaves their next step bit for bit
        what it is without it; then one ``bioim_joint_reaction`` launch with
        the model's contact on.  All of it is enqueued on the env's stream: no
        host round trip and no synchronization (ids given as a list or array
        are checked on the host; a device tensor of ids is copied back once
        for the check).  Two exceptions: an env that has had an RK budget
        (``set_rk_budget``) realizes through ``osim``, which reads its
        suspended-step flags back, and a precision=32 env's first call uploads
        the fp64 model image.  ``rows``: state rows already gathered for these
        envs.  The result labels itself for ``joint_reaction.write_sto``."""
        from . import joint_reaction as jr
        pk = self.pack
        jr.check_frame(frame, on)
        n, q, u, realize = self._own_state_inputs(env_ids, rows)
        _, want = jr.check_args(pk.ndof, pk.nmuscle, pk.ncbody, q, u, want=want, frame=frame, on=on)
        if q.shape[0] != n:
            raise ValueError(f'joint_reaction: rows has {q.shape[0]} rows for {n} envs')
        qdd = ft = None
        if n:
            rep = realize()
            qdd, ft = rep['qdd'], rep['ft']
        if getattr(self, '_jr_table', None) is None:
            self._jr_table = jr.JointTable(self.env_id)
        ext = self.external_wrench_ground(env_ids, rows) if n and self.external_forces is not None else None
        res = jr.Result(jr.launch(self, q, u, qdd, ft, ext, True, frame, on, want))
        res.table, res.frame, res.on = self._jr_table, frame, on
        return res

    def induced_accelerations(self, env_ids=None, kind='point', want=('accel',), force_threshold=0.0, rows=None):
        """Induced accelerations (``bioimitation.induced_accelerations``) at
        the envs' own state: {key: device tensor} for the keys of ``want``,
        one row per env (or per listed env, in the list's order; distinct
        ids), one column per contributor.  Built like ``joint_reaction``: q and
        u are gathered on the device (``state_rows``); the muscles' tendon
        forces and the actuators' forces come from a REALIZE report of those
        envs (``bioim_realize_report``, which leaves their next step bit for
        bit what it is without it), the actuator forces mapped to the dofs
        through the pack's coordinate-actuator table; then one
        ``bioim_induced_accel`` launch in which the model itself decides which
        feet are held (``kind='point'``, ``force_threshold``).  All of it is
        enqueued on the env's stream: no host round trip and no
        synchronization (an env that has had an RK budget realizes through
        ``osim``, which reads its suspended-step flags back).  fp64 envs only.
        ``rows``: state rows already gathered for these envs."""
        import torch
        from . import induced_accelerations as ia
        pk = self.pack
        ia.check_env(self)
        n, q, u, realize = self._own_state_inputs(env_ids, rows)
        _, want = ia.check_args(pk.ndof, pk.nmuscle, pk.ncbody, pk.ncforce, q, u, kind=kind,
                                force_threshold=force_threshold, want=want)
        if q.shape[0] != n:
            raise ValueError(f'induced_accelerations: rows has {q.shape[0]} rows for {n} envs')
        ft = tau_act = None
        if n:
            rep = realize()
            ft = rep['ft']
            if pk.ncoordact:
                if getattr(self, '_ia_act_dof', None) is None:
                    # [nact][ndof] 0 / 1: coordinate actuator a drives dof coordact[a].dof (none: a locked coordinate)
                    m = np.zeros((pk.nact, pk.ndof))
                    for a in range(pk.ncoordact):
                        if pk.coordact[a].dof >= 0:
                            m[a, pk.coordact[a].dof] = 1.0
                    self._ia_act_dof = torch.as_tensor(m).to(device=self.device, dtype=self.dtype, non_blocking=True)
                tau_act = (rep['act'] @ self._ia_act_dof).contiguous()
        ext = self.external_wrench_ground(env_ids, rows) if n and self.external_forces is not None else None
        res = ia.Result(ia.launch(self, q, u, ft, tau_act, ext, kind, None, None, force_threshold, want))
        if getattr(self, '_ia_names', None) is None:
            from .obslayout import load_names
            names = load_names(self.env_id)
            self._ia_names = (ia.contributor_names(pk, names), ia.dof_names(pk, names))
        (res.contributors, res.coords), res.kind = self._ia_names, kind
        return res

    def body_kinematics(self, env_ids=None, qdd=None, points=None, local=False, want=('com', 'system'), rows=None):
        """Body and point kinematics (``bioimitation.body_kinematics``) at the
        envs' own state: {key: device tensor} for the keys of ``want``, one
        row per env (or per listed env, in the list's order; distinct ids).
        q and u are gathered on the device (``state_rows``), then one
        ``bioim_body_kin`` launch on the env's own handle and stream: no host
        round trip and no synchronization (ids given as a list or array are
        checked on the host).  ``qdd``: None (zeros: the accelerations are then
        the velocity terms alone), ``[n][ndof]`` accelerations of the caller's,
        or 'own': the envs' forward-dynamics q'' from a REALIZE report, as
        ``joint_reaction`` takes them.  ``points``: [(body name or 'ground',
        (x, y, z))].  A read: the env state, the next steps' outputs and the
        realize cache stay what they are.  ``rows``: state rows already
        gathered for these envs."""
        from . import body_kinematics as bk
        pk = self.pack
        if getattr(self, '_bk_bodies', None) is None:
            from .obslayout import load_names
            self._bk_bodies = list(load_names(self.env_id)['bodies'])
        n, q, u, realize = self._own_state_inputs(env_ids, rows)
        own = isinstance(qdd, str)
        if own and qdd != 'own':
            raise ValueError(f"body kinematics: qdd must be None, 'own' or [n][ndof] accelerations, got {qdd!r}")
        _, want, pt_body, pt_local = bk.check_args(pk.ndof, self._bk_bodies, q, u, None if own else qdd, points, local,
                                                   want)
        if q.shape[0] != n:
            raise ValueError(f'body_kinematics: rows has {q.shape[0]} rows for {n} envs')
        if own:
            qdd = realize()['qdd'] if n else None
        elif qdd is not None:
            from ._analysis import to_device
            qdd = to_device(qdd, self.device, self.dtype)
        res = bk.Result(bk.launch(self, q, u, qdd, pt_body, pt_local, local, want))
        res.bodies, res.local = self._bk_bodies, bool(local)
        return res

    def load_state(self, rows, env_ids=None):
        """Write flat state rows (``state_rows``' layout: a contiguous
        (n, state_dim) float64 tensor on the env's device) into the listed
        envs, row i into env ``env_ids[i]`` (default: all envs in order), on
        the env's stream without synchronizing (bioim_load_state).  As with
        ``set_state`` the written envs are at a step boundary and their
        realize cache is stale; unlike it, every other env — its realize
        cache included — is left alone."""
        self._bind_stream()
        ids = None
        n = self.num_envs
        if env_ids is not None:
            host, ids = self._id_list(env_ids, 'env', distinct=True)
            n = host.size
        self._check_rows(rows, n, 'load_state: rows')
        if n == 0:
            return
        if env_ids is not None and ids is None:
            ids = self._upload_ids(host)
        _lib.check(self._L.bioim_load_state(self._h, self._ptr(ids), n, self._ptr(rows)))

    def clone_envs(self, src, dst):
        """Make every env of ``dst`` an exact copy of its ``src`` env (an int:
        one source for all; or one id per dst), in one launch on the env's
        stream (bioim_clone_envs).  The whole per-env record travels — also
        what the flat state row lacks: the fiber-velocity warm starts, the
        realize-cache row and a suspended RK step — so a clone continues bit
        for bit like its source under the same actions.  Reset and RK
        counters stay with their envs.  ``dst`` ids are distinct and none is
        also a source."""
        self._bind_stream()
        dst_h, dst_d = self._id_list(dst, 'dst', distinct=True)
        n = dst_h.size
        if isinstance(src, (int, np.integer)):
            src = np.full(n, int(src), dtype=np.int64)
        src_h, src_d = self._id_list(src, 'src', distinct=False)
        if src_h.size != n:
            raise ValueError(f'clone_envs: {src_h.size} src ids for {n} dst ids')
        if np.intersect1d(src_h, dst_h).size:
            raise ValueError('clone_envs: an env cannot be both a src and a dst')
        if n == 0:
            return
        if src_d is None or dst_d is None:     # one upload for both lists
            both = self._upload_ids(np.stack([src_h, dst_h]))
            src_d, dst_d = both[0], both[1]
        _lib.check(self._L.bioim_clone_envs(self._h, self._ptr(src_d), self._ptr(dst_d), n))

    def set_state(self, s: np.ndarray):
        s = np.ascontiguousarray(s, dtype=np.float64)
        assert s.shape == (self.num_envs, self.state_dim)
        _lib.check(self._L.bioim_set_state(self._h, s.ctypes.data_as(C.POINTER(C.c_double))))

    def debug_plane(self, name, data=None):
        """Debug / tests (``bioim_debug_plane``): one whole plane of the
        per-env record (a ``DState`` member, by name) as a numpy array —
        ``(count, N)`` with the env index fastest, ``(N, cache_dim)`` for the
        realize cache, in the env's precision for the real-valued planes.
        ``data``: write that array into the plane instead.  Synchronizes the
        env's streams.  The library refuses a size that is not the plane's."""
        pk, n = self.pack, self.num_envs
        real = np.float32 if self.precision == 32 else np.float64
        nd, nm1, na, na1 = pk.ndof, max(pk.nmuscle, 1), pk.nact, max(pk.nact, 1)
        from .packdef import MAX_HORIZON
        shapes = {'q': (real, nd), 'u': (real, nd), 'act': (real, nm1), 'lce': (real, nm1),
                  'hist': (real, MAX_HORIZON * na), 'last': (real, na), 'old_px': (real, 1), 't': (np.float64, 1),
                  'istep': (np.int32, 1), 'has_last': (np.int32, 1), 'done': (np.int32, 1), 'resets': (np.int32, 1),
                  'hrk': (np.float64, 1), 'pend': (np.int32, 1), 'rkt': (np.float64, 1), 'rkh': (np.float64, 1),
                  'rka': (np.int32, 1), 'ctl': (real, na1), 'cur': (real, na1), 'vnw': (real, nm1),
                  'rkev': (np.uint64, 1)}
        if name == 'cache':     # CacheLay: packed lower system, right-hand side, 3 per muscle, h
            dtype, shape = real, (n, nd * (nd + 1) // 2 + nd + 3 * pk.nmuscle + 1)
        elif name == 'cache_ok':
            dtype, shape = np.int32, (1, n)
        elif name in shapes:
            dtype, shape = shapes[name][0], (shapes[name][1], n)
        else:
            raise ValueError(f'no state plane named {name!r}')
        if data is None:
            out = np.zeros(shape, dtype=dtype)
            _lib.check(self._L.bioim_debug_plane(self._h, name.encode(), out.ctypes.data_as(C.c_void_p), out.nbytes, 0))
            return out
        arr = np.ascontiguousarray(data, dtype=dtype)
        if arr.shape != shape:
            raise ValueError(f'plane {name} has shape {shape}, got {arr.shape}')
        _lib.check(self._L.bioim_debug_plane(self._h, name.encode(), arr.ctypes.data_as(C.c_void_p), arr.nbytes, 1))

    def reset_count(self) -> int:
        """Resets so far over all envs (explicit + in-kernel auto-resets)."""
        n = C.c_uint64()
        _lib.check(self._L.bioim_reset_count(self._h, C.byref(n)))
        return int(n.value)

    def eval_count(self) -> int:
        """Dynamics evaluations of the adaptive integrator so far over all envs
        (bioim_eval_count)."""
        n = C.c_uint64()
        _lib.check(self._L.bioim_eval_count(self._h, C.byref(n)))
        return int(n.value)

    def finished_count(self) -> int:
        """Env steps the adaptive integrator finished so far over all envs
        (bioim_finished_count: the rows whose ``ready`` was 1)."""
        n = C.c_uint64()
        _lib.check(self._L.bioim_finished_count(self._h, C.byref(n)))
        return int(n.value)

    def set_rk_counters(self, evals: int = 0, finished: int = 0):
        """Set every env's evaluation / finished-step counters
        (bioim_set_rk_counters; 32 bits each per env, wrapping independently)."""
        _lib.check(self._L.bioim_set_rk_counters(self._h, int(evals) & 0xffffffff, int(finished) & 0xffffffff))

    def sync(self):
        _lib.check(self._L.bioim_sync(self._h))

    def close(self):
        if getattr(self, '_h', None):
            self._L.bioim_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MixedVectorEnv:
    """A batch of several env IDs on one GPU (BASELINE.json config C5:
    MuscleLockedKneeImitation3D-v0 + MusclePalsyImitation3D-v0), stepped by
    ``bioim_step_group``: segment i owns rows [off_i, off_i + n_i) of padded
    buffers — actions (N, max A), obs (N, max O), info (N, max I) — with
    ``action_mask`` / ``obs_mask`` marking each row's valid columns; one
    launch per segment, in order, on the first segment's stream.
    Device-drawn reset rows are keyed by the global env index (``env_offset``
    + row), as in :class:`VectorEnv`, so the batch reproduces each segment
    stepped alone bit for bit.  ``rollout`` runs T such steps from an action
    plan in one call (``bioim_rollout_group``); per-env resets, the active
    mask and the state calls (``state_rows``, ``load_state``, ``clone_envs``)
    take global env ids and dispatch to the segments."""

    def __init__(self, segments, config=None, device: int = 0, precision: int = 64, seed: int = 0,
                 auto_reset: bool = False, env_offset: int = 0):
        if 'reference' in (config or {}):
            raise ValueError("MixedVectorEnv: config['reference'] holds one model's reference motion (its coordinates "
                             'and bodies); a mixed batch takes no run-time reference')
        import torch
        self.envs, off = [], 0
        for env_id, n in segments:
            self.envs.append(VectorEnv(env_id, n, config=config, device=device, precision=precision, seed=seed,
                                       auto_reset=auto_reset, env_offset=env_offset + off))
            off += int(n)
        self.num_envs = off
        self.device, self.dtype, self.precision = self.envs[0].device, self.envs[0].dtype, precision
        self.action_dim = max(e.action_dim for e in self.envs)
        self.obs_dim = max(e.obs_dim for e in self.envs)
        self.info_dim = max(e.info_dim for e in self.envs)
        n, dev = self.num_envs, self.device
        self.obs = torch.zeros((n, self.obs_dim), dtype=self.dtype, device=dev)
        self.reward = torch.zeros(n, dtype=self.dtype, device=dev)
        self.done = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.info = torch.zeros((n, self.info_dim), dtype=self.dtype, device=dev)
        self.action_mask = torch.zeros((n, self.action_dim), dtype=torch.bool, device=dev)
        self.obs_mask = torch.zeros((n, self.obs_dim), dtype=torch.bool, device=dev)
        self.offsets = []
        off = 0
        for e in self.envs:
            _lib.check(e._L.bioim_set_io_strides(e._h, self.action_dim, self.obs_dim, self.info_dim))
            sl = slice(off, off + e.num_envs)
            e.obs, e.reward, e.done, e.info = self.obs[sl], self.reward[sl], self.done[sl], self.info[sl]
            self.action_mask[sl, :e.action_dim] = True
            self.obs_mask[sl, :e.obs_dim] = True
            self.offsets.append(off)
            off += e.num_envs
        self._hs = (C.c_void_p * len(self.envs))(*[e._h.value for e in self.envs])
        self._L = self.envs[0]._L
        self._auto_reset = bool(auto_reset)

    @property
    def build_id(self) -> str:
        return self._L.bioim_build_id().decode()

    @property
    def last_step_fused(self) -> bool:
        """whether the last ``step`` ran as ONE fused two-topology launch
        (bioim_group_fused) rather than one launch per segment"""
        return _lib.check(self._L.bioim_group_fused(self.envs[0]._h)) == 1

    def _global_ids(self, ids, what, distinct):
        """global env ids (list, range, numpy array or tensor) as a host int64
        array: integers in [0, num_envs), with ``distinct`` not repeating"""
        import torch
        if isinstance(ids, torch.Tensor):
            if ids.dtype in (torch.bool, torch.float16, torch.bfloat16, torch.float32, torch.float64):
                raise ValueError(f'{what} ids must be integers, got {ids.dtype}')
            ids = ids.detach().cpu().numpy()
        host = np.asarray(ids).reshape(-1)
        if host.size and host.dtype.kind not in 'iu':
            raise ValueError(f'{what} ids must be integers, got {host.dtype}')
        host = host.astype(np.int64)
        if host.size and (host.min() < 0 or host.max() >= self.num_envs):
            raise ValueError(f'{what} ids must lie in [0, {self.num_envs})')
        if distinct and np.unique(host).size != host.size:
            raise ValueError(f'{what} ids must be distinct')
        return host

    def _split(self, host):
        """(segment env, positions in the list, segment-local ids) for every
        segment that owns some of the global ids ``host``, in segment order;
        the list's order is kept within a segment"""
        seg = self._segment_of(host)
        for i, e in enumerate(self.envs):
            pos = np.nonzero(seg == i)[0]
            if pos.size:
                yield e, pos, host[pos] - self.offsets[i]

    def _segment_of(self, host):
        """the index of the segment that owns each global id"""
        return np.searchsorted(np.asarray(self.offsets[1:], dtype=np.int64), host, side='right')

    def _upload_index(self, host):
        """host positions as an int64 device tensor, copied from pinned memory
        on the current stream without waiting for the device"""
        import torch
        return torch.from_numpy(np.ascontiguousarray(host, dtype=np.int64)).pin_memory().to(self.device, non_blocking=True)

    def reset(self, env_ids=None, ref_index=None):
        """Reset the listed envs (global ids; default all).  ref_index: one
        reference row per listed env (default: drawn on the device).  Each
        segment resets its own envs, as ``VectorEnv.reset``."""
        if env_ids is None and ref_index is None:
            for e in self.envs:
                e.reset()
            return self.obs
        host = np.arange(self.num_envs, dtype=np.int64) if env_ids is None else self._global_ids(env_ids, 'env', distinct=True)
        rows = None
        if ref_index is not None:
            rows = np.asarray(ref_index.detach().cpu().numpy() if hasattr(ref_index, 'detach') else ref_index).reshape(-1)
            if rows.size != host.size:
                raise ValueError(f'reset: {rows.size} ref_index rows for {host.size} envs')
        for e, pos, local in self._split(host):
            e.reset(local, None if rows is None else rows[pos])
        return self.obs

    def set_auto_reset(self, on: bool):
        for e in self.envs:
            e.set_auto_reset(on)
        self._auto_reset = bool(on)

    def set_external_forces(self, segment, points, wrench=None, point_in='body'):
        """External body forces on one segment (``VectorEnv.set_external_forces``
        of ``self.envs[segment]``: its own body names and (n_segment, K, 9)
        tensor, which is returned).  With forces on either segment the group
        steps and rolls out with one launch per segment."""
        return self.envs[segment].set_external_forces(points, wrench, point_in)

    def set_active_mask(self, mask):
        """Per-env step mask over the whole batch: a (N,) uint8/bool device
        tensor (``check_env_mask``), handed to the segments' handles in
        slices; ``None`` steps all.  The tensor must stay alive while set."""
        check_env_mask(mask, self.num_envs, self.device)
        self._active = mask
        for e, off in zip(self.envs, self.offsets):
            e.set_active_mask(None if mask is None else mask[off:off + e.num_envs])

    @property
    def state_dim(self) -> int:
        """width of the padded state rows: the largest of the segments'"""
        return max(e.state_dim for e in self.envs)

    @property
    def state_mask(self):
        """(N, state_dim) bool: each row's valid columns (its segment's own state_dim)"""
        import torch
        m = torch.zeros((self.num_envs, self.state_dim), dtype=torch.bool, device=self.device)
        for e, off in zip(self.envs, self.offsets):
            m[off:off + e.num_envs, :e.state_dim] = True
        return m

    _check_rows = VectorEnv._check_rows      # uses only state_dim and device

    def state_rows(self, out=None, env_ids=None):
        """The flat state rows of the listed envs (global ids; default all) as
        (n, state_dim) float64, in the list's order, each row zero-padded past
        its segment's own state_dim (``state_mask``).  One
        ``bioim_copy_state_rows`` launch per segment on the shared stream; no
        synchronization."""
        import torch
        host = np.arange(self.num_envs, dtype=np.int64) if env_ids is None else self._global_ids(env_ids, 'env', distinct=False)
        n, sd = host.size, self.state_dim
        if out is None:
            out = torch.zeros((n, sd), dtype=torch.float64, device=self.device)
        else:
            self._check_rows(out, n, 'state_rows: out')
        for e, pos, local in self._split(host):
            rows = e.state_rows(env_ids=local)
            at = self._upload_index(pos)
            out[at, :e.state_dim] = rows
            if e.state_dim < sd:
                out[at, e.state_dim:] = 0
        return out

    def load_state(self, rows, env_ids=None):
        """Write padded state rows (``state_rows``' layout) into the listed
        envs (global, distinct ids; default all in order): one
        ``bioim_load_state`` launch per segment on the shared stream; no
        synchronization.  Columns past a segment's state_dim are ignored."""
        host = np.arange(self.num_envs, dtype=np.int64) if env_ids is None else self._global_ids(env_ids, 'env', distinct=True)
        self._check_rows(rows, host.size, 'load_state: rows')
        for e, pos, local in self._split(host):
            sub = rows.index_select(0, self._upload_index(pos))[:, :e.state_dim].contiguous()
            e.load_state(sub, local)

    def clone_envs(self, src, dst):
        """``VectorEnv.clone_envs`` with global ids: every dst env becomes an
        exact copy of its src env (an int: one source for all), one
        ``bioim_clone_envs`` launch per segment.  A pair must lie in one
        segment (the records of two env IDs differ): else ``ValueError``."""
        dst_h = self._global_ids(dst, 'dst', distinct=True)
        if isinstance(src, (int, np.integer)):
            src = np.full(dst_h.size, int(src), dtype=np.int64)
        src_h = self._global_ids(src, 'src', distinct=False)
        if src_h.size != dst_h.size:
            raise ValueError(f'clone_envs: {src_h.size} src ids for {dst_h.size} dst ids')
        if np.intersect1d(src_h, dst_h).size:
            raise ValueError('clone_envs: an env cannot be both a src and a dst')
        if np.any(self._segment_of(src_h) != self._segment_of(dst_h)):
            raise ValueError('clone_envs: a src and its dst must lie in one segment')
        for e, pos, local in self._split(dst_h):
            e.clone_envs(src_h[pos] - e.env_offset + self.envs[0].env_offset, local)

    def rollout(self, actions, steps=None, *, obs='last', info=False, stop_at_done=False, out=None):
        """``VectorEnv.rollout`` for the mixed batch (``bioim_rollout_group``):
        T consecutive env steps from an action sequence, enqueued by one call,
        bit for bit what T ``step()`` calls give.  N is the batch total and A,
        O, I the padded widths: ``actions`` (T, N, A), or (N, A) with
        ``steps=T``; ``obs`` 'last' (written to ``self.obs``), 'all'
        ((T, N, O); ``self.obs`` gets the last rows too) or None; ``info``:
        also the (T, N, I) rows; ``stop_at_done`` (auto-reset off only) per
        env, each segment's active mask honoured and left alone; ``out``: a
        dict of caller buffers ('reward' (T, N), 'done' (T, N) uint8, 'obs',
        'info').  Buffers allocated here are zero-filled, so the padding
        columns are zero; those of caller buffers are left alone.  With two
        segments of a fused pair in the default step configuration the call
        is ONE kernel launch, otherwise T group steps enqueued from C — see
        ``last_rollout_fused``.

        Returns (obs, reward (T, N), done (T, N) uint8, info or None)."""
        a, T, stride, buf = _rollout_buffers(self, actions, steps, obs, info,
                                             stop_at_done and any(e._auto_reset for e in self.envs), out, zero=True)
        obs_seq, obs_last = buf.get('obs'), (self.obs if obs is not None else None)
        for e in self.envs:
            if getattr(e, '_storage_grow', 0):
                e._apply_storage_growth()
        p = VectorEnv._ptr
        self.envs[0]._bind_stream()      # as step(): the call is ordered on segment 0's stream
        _lib.check(self._L.bioim_rollout_group(self._hs, len(self.envs), p(a), T, stride, p(obs_seq), p(obs_last),
                                               p(buf['reward']), p(buf['done']), p(buf.get('info')),
                                               1 if stop_at_done else 0))
        return (self.obs if obs == 'last' else obs_seq), buf['reward'], buf['done'], buf.get('info')

    @property
    def last_rollout_fused(self) -> bool:
        """True if the last ``rollout()`` ran as ONE launch of the
        two-topology rollout kernel, False if it looped over the group steps
        (bioim_rollout_group_fused)."""
        return bool(_lib.check(self._L.bioim_rollout_group_fused(self.envs[0]._h)))

    def step(self, actions):
        """actions: (N, max A) tensor; columns beyond a row's own action dim are ignored."""
        a = actions
        if a.dtype != self.dtype or a.device != self.device or not a.is_contiguous():
            a = a.to(device=self.device, dtype=self.dtype).contiguous()
        assert a.shape == (self.num_envs, self.action_dim), a.shape
        p = VectorEnv._ptr
        self.envs[0]._bind_stream()      # segment 0 launches on it; the others fork from and join into it
        _lib.check(self._L.bioim_step_group(self._hs, len(self.envs), p(a), p(self.obs), p(self.reward),
                                            p(self.done), p(self.info)))
        return self.obs, self.reward, self.done, self.info

    def close(self):
        for e in self.envs:
            e.close()
