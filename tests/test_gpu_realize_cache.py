"""Every path that invalidates the realize cache, and the
cache kept across read-only queries.

A default step's first substep solves the implicit system the previous
launch's realize stored in ``DState::cache`` whenever ``cache_ok[env]`` is set
and the row's ``h`` equals the step's ``dt``.  Every path that moves
q/u/act/lce without forming a new row must clear the flag, or the next step
silently solves a stale system.

The reference for values is a twin ``VectorEnv`` (same seed, reset rows,
actions and intervening operations) whose cache the host drops before every
default step with ``set_state(get_state())`` — a round trip that does not go
through the logic under test.  Bounds, all the project's own: torque models
bit-equal, muscle models within 5e-9 relative on the observation
(test_realize_cache_first_substep's bound; 1.1e-9 observed), and 1e-6 against
the fp64 oracle where it is driven through the same calls (plain steps,
``integrate``).  ``test_a_stale_row_is_visible`` shows that a missed clear
would break the twin bound by orders of magnitude.

32 envs are two 16-env workgroups; SUBSET is half of each.  The planes are
read and written with ``VectorEnv.debug_plane`` (``bioim_debug_plane``)."""
import random

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason='needs a HIP GPU')]

N = 32
BOUND = 5e-9          # muscle models, cached against uncached first substep (tests/test_gpu_parity.py)
ORACLE = 1e-6         # the fp64 step-parity bound (tests/test_gpu_parity.py)
M2D, T2D = 'MuscleWalkingImitation2D-v0', 'TorqueWalkingImitation2D-v0'
M3D, T3D = 'MuscleRunningImitation3D-v0', 'TorqueWalkingImitation3D-v0'
FAMILIES = [M2D, T2D, M3D, T3D]
SUBSET = [e for e in range(N) if e % 16 < 8]
REST = [e for e in range(N) if e % 16 >= 8]
# what a default step reads of an env's record (ctl: written by the step's own actuate first)
READ_PLANES = ('q', 'u', 'act', 'lce', 'hist', 'last', 't', 'istep', 'cache', 'cache_ok')


def _rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def _t(env, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=env.device, dtype=env.dtype)


def _rows(pk, n=N, seed=11):
    """a distinct reference row per env"""
    assert pk.reset_hi + 1 >= n
    return np.random.default_rng(seed).permutation(pk.reset_hi + 1)[:n].astype(np.int32)


def _flags(env):
    return env.debug_plane('cache_ok')[0]


H_COL = -1           # a cache row's last entry is the h its system was formed at (CacheLay::H)


class Drive:
    """Actions for a batch of one env ID: muscle models U[0, 0.3]; torque
    models the reference targets of each env's next row + N(0, 0.02) (the
    actions of tests/test_gpu_state_clone.py).  ``idx`` follows each env's
    reference row through steps, integrates and resets."""

    def __init__(self, pk, rows, seed=12):
        self.pk, self.idx, self.rng = pk, np.array(rows, dtype=np.int64), np.random.default_rng(seed)

    def actions(self):
        pk, n = self.pk, len(self.idx)
        if pk.nmuscle:
            return self.rng.uniform(0.0, 0.3, size=(n, pk.nact))
        base = np.array([[pk.ref_q[min(int(r) + 1, pk.nrows - 1)][pk.pd_coord[a]] for a in range(pk.nact)]
                         for r in self.idx])
        return base + self.rng.normal(0.0, 0.02, size=(n, pk.nact))

    def controls(self, n):
        """held controls for an OsimModel call: excitations, or torques of the PD law's size"""
        pk = self.pk
        return self.rng.uniform(0.0, 0.3, size=(n, pk.nact)) if pk.nmuscle else self.rng.normal(0.0, 20.0, size=(n, pk.nact))


class Twin:
    """``a``: the env under test.  ``b``: its twin, whose realize cache the
    host drops before every default step.  ``step`` steps both with the same
    actions and compares them under the module's bounds."""

    def __init__(self, env_id, precision=64, rows=None, with_oracle=False):
        from bioimitation.registry import load_pack
        from bioimitation.vector_env import VectorEnv
        self.env_id, self.pk = env_id, load_pack(env_id)
        self.rows = _rows(self.pk) if rows is None else np.asarray(rows, dtype=np.int32)
        self.a = VectorEnv(env_id, N, precision=precision, seed=2)
        self.b = VectorEnv(env_id, N, precision=precision, seed=2)
        assert self.a.launch['envs_per_workgroup'] == 16
        for e in (self.a, self.b):
            e.reset(ref_index=self.rows)
        self.drive = Drive(self.pk, self.rows)
        self.worst, self.worst_orc, self.steps = 0.0, 0.0, 0
        self.orc = None
        if with_oracle:
            import oracle
            self.orc = oracle.Oracle(self.pk)
            self.bufs = self.orc.new_envs(N)
            for i in range(N):
                self.orc.reset(self.bufs, i, int(self.rows[i]))
            self.alive = np.ones(N, bool)

    def both(self, f):
        for e in (self.a, self.b):
            f(e)

    def step(self, act=None, drop=True, compare=True):
        """one step of both envs; ``drop``: the twin's cache is dropped first
        (every default step; get_state refuses envs suspended by an RK budget)"""
        act = self.drive.actions() if act is None else act
        if drop:
            self.b.set_state(self.b.get_state())
        oa = [x.cpu().numpy().copy() for x in self.a.step(_t(self.a, act))]
        ob = [x.cpu().numpy().copy() for x in self.b.step(_t(self.b, act))]
        self.drive.idx += 1
        self.steps += 1
        if compare:
            self.compare(oa, ob)
        if self.orc is not None:
            for i in range(N):
                o, r, d, inf = self.orc.step(self.bufs, i, act[i])
                if self.alive[i]:
                    self.worst_orc = max(self.worst_orc, float(_rel(oa[0][i], o).max()))
                    self.alive[i] = not d
        return oa, ob

    def compare(self, oa, ob):
        what = f'{self.env_id} step {self.steps}'
        d = float(_rel(oa[0], ob[0]).max())
        self.worst = max(self.worst, d)
        print(f'{what}: obs vs twin {d:.2e}, reward {np.abs(oa[1] - ob[1]).max():.2e}, '
              f'info {np.abs(oa[3] - ob[3]).max():.2e}')
        assert np.array_equal(oa[2], ob[2]), what
        if self.pk.nmuscle:
            assert d < BOUND, (what, d)
        else:
            for x, y, name in zip(oa, ob, ('obs', 'reward', 'done', 'info')):
                assert np.array_equal(x, y), (what, name)

    def finish(self):
        print(f'{self.env_id}: {self.steps} steps, worst obs vs twin {self.worst:.2e}'
              + (f', vs oracle {self.worst_orc:.2e} ({int(self.alive.sum())}/{N} alive)' if self.orc else ''))
        if self.orc is not None:
            assert self.worst_orc < ORACLE, self.worst_orc
        self.a.close()
        self.b.close()


def _moved(env, before, ids):
    """the operation moved the state of every listed env (else the case proves nothing)"""
    import torch
    after = env.state_rows()
    for e in ids:
        assert not torch.equal(after[e], before[e]), f'env {e}: the operation left the state as it was'


# ---------------------------------------------------------------- (a) sensitivity

@pytest.mark.parametrize('env_id', FAMILIES)
def test_a_stale_row_is_visible(env_id):
    """What a missed clear looks like.  After 3 steps every env's cache row is
    saved; one more step; the saved rows go back with cache_ok = 1 — the rows
    are now one step stale, as after an operation that moved the state and
    forgot the flag (their h entry is set to the fresh rows', so that the
    first substep's ``cache_h == dt`` test cannot reject them by luck: h is
    (step_size * (istep + 1) - t) / nsub and varies in its last bits from step
    to step).  The next observation must differ from the twin's by at least
    100 x the 5e-9 the interleaving tests below allow.

    Measured on an MI355X (max over 32 envs, relative to max(1, |x|)):
    MuscleWalking2D 4.2e+01, TorqueWalking2D 1.8e+00, MuscleRunning3D 4.5e+00,
    TorqueWalking3D 2.2e+00; the least affected env of each batch 4.2e-02,
    8.1e-04, 5.2e-02 and 5.8e-03 — every one at least 1.6e5 x the bound."""
    k = Twin(env_id)
    for _ in range(3):
        k.step()
    saved = k.a.debug_plane('cache')
    k.step()
    fresh = k.a.debug_plane('cache')
    assert (_flags(k.a) == 1).all()
    assert not np.array_equal(saved, fresh)
    stale = saved.copy()
    stale[:, H_COL] = fresh[:, H_COL]
    k.a.debug_plane('cache', stale)
    k.a.debug_plane('cache_ok', np.ones((1, N), np.int32))
    oa, ob = k.step(compare=False)
    d = _rel(oa[0], ob[0]).max(axis=1)
    print(f'{env_id}: one-step-stale cache rows change the next observation by {d.max():.2e} '
          f'(smallest over the envs {d.min():.2e}); the twin bound is {BOUND:.0e}')
    assert d.max() >= 100 * BOUND, d.max()
    k.a.close()
    k.b.close()


# ---------------------------------------------------------------- (b) the cached path runs

@pytest.mark.parametrize('env_id', FAMILIES)
def test_b_swapped_rows_show_the_cached_path_runs(env_id):
    """Envs 3 and 20 (different workgroups) start at the same reference row —
    same t and istep, so the same h — and get different actions for 3 steps.
    Their cache rows are swapped, flags kept at 1: both next observations must
    leave the twin's (by more than the twin bound), so the first substep
    really solved the row — torque models included, where a cached and an
    uncached first substep give the same bits and a cache that is never used
    would go unnoticed.  With the flags written to 0 instead the swapped rows
    are ignored: the outputs equal the twin's again."""
    from bioimitation.registry import load_pack
    i, j = 3, 20
    rows = _rows(load_pack(env_id))
    rows[j] = rows[i]
    for flag in (1, 0):
        k = Twin(env_id, rows=rows)
        for _ in range(3):
            k.step()
        c = k.a.debug_plane('cache')
        assert c[i, H_COL] == c[j, H_COL] and not np.array_equal(c[i], c[j])
        c[[i, j]] = c[[j, i]]
        k.a.debug_plane('cache', c)
        f = _flags(k.a)
        assert (f == 1).all()
        f[[i, j]] = flag
        k.a.debug_plane('cache_ok', f[None, :])
        oa, ob = k.step(compare=(flag == 0))
        d = _rel(oa[0], ob[0]).max(axis=1)
        print(f'{env_id}: swapped rows, flags {flag}: obs vs twin env {i} {d[i]:.2e}, env {j} {d[j]:.2e}, '
              f'others {np.delete(d, [i, j]).max():.2e}')
        if flag:
            assert d[i] > BOUND and d[j] > BOUND, (d[i], d[j])
            others = [e for e in range(N) if e not in (i, j)]
            k.compare([x[others] for x in oa], [x[others] for x in ob])
        assert (_flags(k.a) == 1).all()
        k.finish()


# ---------------------------------------------------------------- (c) + (d) interleavings

def _op_integrate(k):
    ctl = k.drive.controls(len(SUBSET))
    k.both(lambda e: e.osim('integrate', SUBSET, controls=ctl))
    k.drive.idx[SUBSET] += 1
    if k.orc is not None:
        for r, i in enumerate(SUBSET):
            k.orc.osim_actuate(k.bufs, i, ctl[r])
            k.orc.osim_integrate(k.bufs, i)
    return SUBSET


def _op_equilibrate(k):
    k.both(lambda e: e.osim('equilibrate', SUBSET))
    return SUBSET


def _op_reset_subset(k):
    rows = _rows(k.pk, len(SUBSET), seed=13)
    k.both(lambda e: e.reset(env_ids=SUBSET, ref_index=rows))
    k.drive.idx[SUBSET] = rows
    return SUBSET


@pytest.mark.parametrize('env_id,op', [(e, 'integrate') for e in FAMILIES] + [(e, 'equilibrate') for e in (M2D, M3D)] +
                         [(e, 'reset') for e in FAMILIES])
def test_d_osim_call_or_subset_reset_between_steps(env_id, op):
    """3 default steps, then on half the envs ``osim('integrate', controls)``,
    ``osim('equilibrate')`` or ``reset(env_ids, ref_index)``, then 3 default
    steps.  After a step every flag is 1; after an OsimModel call the moved
    envs' flags are 0; a subset reset leaves every flag at 1 (it forms the
    reset envs' rows and touches no other env).  The plain steps and the
    integrate are also held against the oracle."""
    import torch
    k = Twin(env_id, with_oracle=(op == 'integrate'))
    assert (_flags(k.a) == 1).all(), 'a reset forms the cache row'
    for _ in range(3):
        k.step()
        assert (_flags(k.a) == 1).all()
    before = k.a.state_rows().clone()
    rows_before = k.a.debug_plane('cache')
    moved = {'integrate': _op_integrate, 'equilibrate': _op_equilibrate, 'reset': _op_reset_subset}[op](k)
    _moved(k.a, before, moved)
    assert torch.equal(k.a.state_rows()[REST], before[REST])
    f = _flags(k.a)
    if op == 'reset':
        assert (f == 1).all(), f
        rows_after = k.a.debug_plane('cache')
        assert np.array_equal(rows_after[REST], rows_before[REST])
        assert all(not np.array_equal(rows_after[e], rows_before[e]) for e in moved)
    else:
        assert (f[moved] == 0).all(), f
    for _ in range(3):
        k.step()
        assert (_flags(k.a) == 1).all()
    k.finish()


@pytest.mark.parametrize('env_id', FAMILIES)
def test_d_push_step_between_default_steps(env_id):
    """3 default steps; a torso push table (+-50 N, never 0) is installed and
    one step runs with it (the push kernel, which forms no cache row); the
    table is removed (npts = 0) and 3 default steps follow.  After the push
    step every flag is 0, and the first default step after it runs without
    the cache."""
    k = Twin(env_id)
    for _ in range(3):
        k.step()
    rng = np.random.default_rng(9)
    x = np.arange(0.0, 4.0, 0.03) + 0.0013
    y = rng.choice([-50.0, 50.0], size=(N, len(x)))
    k.both(lambda e: e.set_perturbation(x, y))
    # the push is live: a third env without it ends the same step elsewhere
    from bioimitation.vector_env import VectorEnv
    free = VectorEnv(env_id, N, precision=64, seed=2)
    free.load_state(k.a.state_rows())
    act = k.drive.actions()
    o_free = free.step(_t(free, act))[0].cpu().numpy().copy()
    free.close()
    before = k.a.state_rows().clone()
    oa, _ = k.step(act)
    assert (_rel(oa[0], o_free).max(axis=1) > 1e-6).all(), 'the push changed nothing for some env'
    _moved(k.a, before, range(N))
    assert (_flags(k.a) == 0).all()
    k.both(lambda e: e.set_perturbation(None, None))      # bioim_set_perturbation with npts = 0
    for _ in range(3):
        k.step()
        assert (_flags(k.a) == 1).all()
    k.finish()


@pytest.mark.parametrize('budget', [0, 2])
@pytest.mark.parametrize('env_id', FAMILIES)
def test_d_rk_merson_between_default_steps(env_id, budget):
    """3 default steps; the handle switches to RK-Merson (bioim_set_integrator,
    with and without a budget of 2 attempts per launch) and steps until no
    env is suspended; back to the semi-implicit substeps for 3 default steps.
    After the RK launches every flag is 0.

    The twin takes the tested env's flat state (host get_state / set_state)
    just before the switch.  The two are a rounding error apart by then (the
    cached against the uncached first substeps), and one adaptive step at
    accuracy 1e-3 amplifies that: without the re-sync MuscleRunning3D came out
    of the RK step 2.4e-7 from its twin on an MI355X, the distance
    test_rk_merson_parity_fp64 allows between the GPU and the oracle after one
    RK step (2.2e-7 observed there) and 48 x the 5e-9 the default steps after
    it are held to.  From the same bits the RK kernels give the same bits
    (asserted), so what the default steps after the switch compare is the
    cache logic alone, under the unchanged bound."""
    import torch
    from bioimitation import _lib
    k = Twin(env_id)
    for _ in range(3):
        k.step()
    before = k.a.state_rows().clone()
    k.b.set_state(k.a.get_state())
    ready = {}
    for e in (k.a, k.b):
        _lib.check(e._L.bioim_set_integrator(e._h, 1, 1e-3))
        if budget:
            ready[e] = torch.ones(N, dtype=torch.uint8, device=e.device)
            _lib.check(e._L.bioim_set_rk_budget(e._h, budget, e._ptr(ready[e])))
    act = k.drive.actions()
    launches = 0
    none = {e: torch.zeros(N, dtype=torch.uint8, device=e.device) for e in (k.a, k.b)}
    while True:
        # one env step: after the first launch nobody is active, so only the envs it suspended go
        # on (a ready env would start its next step); outputs are compared once all have finished
        oa = [x.cpu().numpy().copy() for x in k.a.step(_t(k.a, act))]
        ob = [x.cpu().numpy().copy() for x in k.b.step(_t(k.b, act))]
        launches += 1
        pa, pb = k.a.pending_count(), k.b.pending_count()
        assert pa == pb, (pa, pb)
        if pa == 0:
            break
        assert launches < 200, 'the RK step did not finish'     # 36 launches on Torque3D at 2 attempts each
        if launches == 1:
            k.both(lambda e: e.set_active_mask(none[e]))
    assert budget == 0 or launches > 1, 'no env was suspended: the budgeted path did not run'
    k.both(lambda e: e.set_active_mask(None))
    k.drive.idx += 1
    k.steps += 1
    print(f'{env_id}: RK step in {launches} launches')
    # every env's output rows were written by the launch it finished in
    for x, y, name in zip(oa + [k.a.state_rows().cpu().numpy()], ob + [k.b.state_rows().cpu().numpy()],
                          ('obs', 'reward', 'done', 'info', 'state rows')):
        assert np.array_equal(x, y), (env_id, name, 'the RK step is not bit-equal from equal states')
    _moved(k.a, before, range(N))
    assert (_flags(k.a) == 0).all()
    for e in (k.a, k.b):
        if budget:
            _lib.check(e._L.bioim_set_rk_budget(e._h, 0, None))
        _lib.check(e._L.bioim_set_integrator(e._h, 0, 0.0))
    for _ in range(3):
        k.step()
        assert (_flags(k.a) == 1).all()
    k.finish()


@pytest.mark.parametrize('env_id', FAMILIES)
def test_d_active_mask_and_load_state(env_id):
    """3 default steps; half the envs are masked for 2 steps, and between
    those two steps load_state writes another env's flat row into one masked
    env (17); unmask; 3 default steps.  A masked step leaves a masked env's
    flag and cache row byte-identical — env 17's flag, which load_state had
    just cleared, is still 0 after it, and no other flag moved."""
    import torch
    k = Twin(env_id)
    for _ in range(3):
        k.step()
    masked, src, dst = SUBSET, 9, 17
    assert dst in masked and src not in masked
    mask = {e: torch.ones(N, dtype=torch.uint8, device=e.device) for e in (k.a, k.b)}
    for e in (k.a, k.b):
        mask[e][masked] = 0
        e.set_active_mask(mask[e])
    rows0, state0 = k.a.debug_plane('cache'), k.a.state_rows().clone()
    oa, ob = k.step(compare=False)
    k.compare([x[REST] for x in oa], [x[REST] for x in ob])
    assert (_flags(k.a) == 1).all()
    assert np.array_equal(k.a.debug_plane('cache')[masked], rows0[masked])
    assert torch.equal(k.a.state_rows()[masked], state0[masked])
    k.both(lambda e: e.load_state(e.state_rows(env_ids=[src]), [dst]))
    _moved(k.a, state0, [dst])
    want = np.ones(N, np.int32)
    want[dst] = 0
    assert np.array_equal(_flags(k.a), want), 'load_state clears the listed env only'
    rows1, state1 = k.a.debug_plane('cache'), k.a.state_rows().clone()
    oa, ob = k.step(compare=False)
    k.compare([x[REST] for x in oa], [x[REST] for x in ob])
    assert np.array_equal(_flags(k.a), want), 'a masked env keeps its flag, a cleared one too'
    assert np.array_equal(k.a.debug_plane('cache')[masked], rows1[masked])
    assert torch.equal(k.a.state_rows()[masked], state1[masked])
    k.drive.idx[masked] -= 2          # the masked envs did not move
    k.drive.idx[dst] = k.drive.idx[src]
    k.both(lambda e: e.set_active_mask(None))
    for _ in range(3):
        k.step()
        assert (_flags(k.a) == 1).all()
    k.finish()


@pytest.mark.parametrize('env_id,precision', [(M2D, 64), (T3D, 64), (T3D, 32)])
def test_c_load_and_clone_touch_only_the_listed_flags(env_id, precision):
    """load_state(rows, ids) clears the listed envs' flags and no other;
    clone_envs gives each dst its src's flag and cache row (a cleared src
    makes a cleared clone) and touches no other env.  fp32 too."""
    from bioimitation.registry import load_pack
    from bioimitation.vector_env import VectorEnv
    pk = load_pack(env_id)
    rows = _rows(pk)
    env = VectorEnv(env_id, N, precision=precision, seed=2)
    env.reset(ref_index=rows)
    drive = Drive(pk, rows)
    for _ in range(2):
        env.step(_t(env, drive.actions()))
    assert (_flags(env) == 1).all()
    ids = [1, 16, 31]
    env.load_state(env.state_rows(env_ids=[2, 3, 4]), ids)
    want = np.ones(N, np.int32)
    want[ids] = 0
    assert np.array_equal(_flags(env), want)
    c0 = env.debug_plane('cache')
    env.clone_envs([1, 5], [20, 21])          # a cleared src, a valid src
    want[20], want[21] = 0, 1
    assert np.array_equal(_flags(env), want)
    c1 = env.debug_plane('cache')
    assert np.array_equal(c1[20], c0[1]) and np.array_equal(c1[21], c0[5])
    keep = [e for e in range(N) if e not in (20, 21)]
    assert np.array_equal(c1[keep], c0[keep])
    env.step(_t(env, drive.actions()))
    assert (_flags(env) == 1).all()
    env.close()


def test_c_flags_fp32():
    """The flag checks of the interleavings on an fp32 handle
    (TorqueWalkingImitation3D-v0, precision 32): no value bound, flags only."""
    import ctypes as C
    import torch
    from bioimitation import _lib
    from bioimitation.obslayout import load_names
    from bioimitation.perturb import os_body_index
    from bioimitation.registry import load_pack
    from bioimitation.vector_env import VectorEnv
    pk = load_pack(T3D)
    rows = _rows(pk)
    env = VectorEnv(T3D, N, precision=32, seed=2)
    drive = Drive(pk, rows)
    L, h = env._L, env._h

    def step():
        env.step(_t(env, drive.actions()))
        drive.idx += 1

    assert (_flags(env) == 0).all()            # a new handle: nothing formed yet
    env.reset(ref_index=rows)
    assert (_flags(env) == 1).all()
    step()
    assert (_flags(env) == 1).all()
    env.osim('realize', SUBSET)                 # reads only
    env.osim('realize', SUBSET, controls=drive.controls(len(SUBSET)))
    assert (_flags(env) == 1).all()
    env.osim('integrate', SUBSET, controls=drive.controls(len(SUBSET)))
    drive.idx[SUBSET] += 1
    assert (_flags(env)[SUBSET] == 0).all()
    step()
    assert (_flags(env) == 1).all()
    env.reset(env_ids=SUBSET, ref_index=rows[SUBSET])
    drive.idx[SUBSET] = rows[SUBSET]
    assert (_flags(env) == 1).all()
    x = np.arange(0.0, 4.0, 0.03) + 0.0013
    y = np.random.default_rng(9).choice([-50.0, 50.0], size=(N, len(x)))
    dp = C.POINTER(C.c_double)
    _lib.check(L.bioim_set_perturbation(h, os_body_index(load_names(T3D), 'torso'), len(x), x.ctypes.data_as(dp),
                                        y.ctypes.data_as(dp)))
    step()
    assert (_flags(env) == 0).all()
    _lib.check(L.bioim_set_perturbation(h, -1, 0, None, None))
    step()
    assert (_flags(env) == 1).all()
    _lib.check(L.bioim_set_integrator(h, 1, 1e-3))
    step()
    assert (_flags(env) == 0).all()
    _lib.check(L.bioim_set_integrator(h, 0, 0.0))
    step()
    assert (_flags(env) == 1).all()
    mask = torch.ones(N, dtype=torch.uint8, device=env.device)
    mask[SUBSET] = 0
    env.set_active_mask(mask)
    env.load_state(env.state_rows(env_ids=[9]), [17])      # 17 is masked
    want = np.ones(N, np.int32)
    want[17] = 0
    rows0 = env.debug_plane('cache')
    step()
    assert np.array_equal(_flags(env), want)
    assert np.array_equal(env.debug_plane('cache')[SUBSET], rows0[SUBSET])
    env.set_active_mask(None)
    env.set_state(env.get_state())
    assert (_flags(env) == 0).all()
    env.close()


@pytest.mark.parametrize('fusion', [1, 0])
def test_d_mixed_batch_integrate_between_group_steps(fusion):
    """MixedVectorEnv, 16 LockedKnee3D + 16 Palsy3D envs, as one fused launch
    (group fusion on) and as side-stream launches (off): 3 group steps,
    ``osim('integrate')`` on half of segment 1 through its own handle, 3 group
    steps, against a twin group whose segments' caches the host drops before
    every step.  The integrate clears the moved envs' flags on segment 1 and
    leaves segment 0's at 1."""
    from bioimitation import _lib
    from bioimitation.registry import load_pack
    from bioimitation.vector_env import MixedVectorEnv
    segs = [('MuscleLockedKneeImitation3D-v0', 16), ('MusclePalsyImitation3D-v0', 16)]
    half = list(range(8))
    L = _lib.load()
    L.bioim_set_group_fusion(fusion)
    try:
        a = MixedVectorEnv(segs, precision=64, seed=2)
        b = MixedVectorEnv(segs, precision=64, seed=2)
        for (env_id, n), ea, eb in zip(segs, a.envs, b.envs):
            rows = _rows(load_pack(env_id), n)
            ea.reset(ref_index=rows)
            eb.reset(ref_index=rows)
        rng = np.random.default_rng(12)
        worst = 0.0

        def step(t):
            nonlocal worst
            act = rng.uniform(0.0, 0.3, size=(a.num_envs, a.action_dim))
            for e in b.envs:
                e.set_state(e.get_state())
            oa = [x.cpu().numpy().copy() for x in a.step(_t(a, act))]
            ob = [x.cpu().numpy().copy() for x in b.step(_t(b, act))]
            assert a.last_step_fused == bool(fusion) and b.last_step_fused == bool(fusion)
            d = float(_rel(oa[0], ob[0]).max())
            worst = max(worst, d)
            print(f'mixed, fusion {fusion}, step {t}: obs vs twin {d:.2e}')
            assert d < BOUND and np.array_equal(oa[2], ob[2]), (t, d)
            for e in a.envs:
                assert (_flags(e) == 1).all()

        for t in range(3):
            step(t)
        before = a.envs[1].state_rows().clone()
        ctl = rng.uniform(0.0, 0.3, size=(len(half), a.envs[1].action_dim))
        for m in (a, b):
            m.envs[1].osim('integrate', half, controls=ctl)
        _moved(a.envs[1], before, half)
        assert (_flags(a.envs[1])[half] == 0).all()
        assert (_flags(a.envs[0]) == 1).all()
        for t in range(3, 6):
            step(t)
        print(f'mixed, fusion {fusion}: worst obs vs twin {worst:.2e}')
        a.close()
        b.close()
    finally:
        L.bioim_set_group_fusion(1)


# ---------------------------------------------------------------- (e) read-only queries

@pytest.mark.parametrize('env_id', FAMILIES)
def test_e_read_only_queries_are_invisible(env_id):
    """Between every pair of steps run A realizes every env, realizes half of
    them with controls and gathers the state rows; run A' does none of it.
    Observation, reward, done, info and the final state rows are bit-identical:
    a query that reads does not change the trajectory.  Each realize leaves
    every plane a default step reads byte-identical (the one with controls
    writes ctl, which the step's own actuate replaces)."""
    import torch
    from bioimitation.registry import load_pack
    from bioimitation.vector_env import VectorEnv
    pk = load_pack(env_id)
    rows = _rows(pk)
    a = VectorEnv(env_id, N, precision=64, seed=2)
    p = VectorEnv(env_id, N, precision=64, seed=2)
    a.reset(ref_index=rows)
    p.reset(ref_index=rows)
    drive = Drive(pk, rows)
    T = 6
    for t in range(T):
        act = drive.actions()
        drive.idx += 1
        oa = a.step(_t(a, act))
        op = p.step(_t(p, act))
        for x, y, name in zip(oa, op, ('obs', 'reward', 'done', 'info')):
            assert torch.equal(x, y), (env_id, t, name, float((x.double() - y.double()).abs().max()))
        if t == T - 1:
            break
        planes = {n: a.debug_plane(n) for n in READ_PLANES}
        ctl = a.debug_plane('ctl')
        a.osim('realize', list(range(N)))
        for n in READ_PLANES + ('ctl',):
            assert np.array_equal(a.debug_plane(n), planes[n] if n != 'ctl' else ctl), (env_id, t, n, 'realize')
        a.osim('realize', SUBSET, controls=drive.controls(len(SUBSET)))
        for n in READ_PLANES:
            assert np.array_equal(a.debug_plane(n), planes[n]), (env_id, t, n, 'realize with controls')
        assert not np.array_equal(a.debug_plane('ctl'), ctl)
        a.state_rows()
        assert (_flags(a) == 1).all()
    assert torch.equal(a.state_rows(), p.state_rows())
    a.close()
    p.close()


def test_e_facade_get_state_dict_between_steps_is_invisible():
    """The single-env facade: make('MuscleWalkingImitation2D-v0') stepped with
    and without get_state_dict() (the calc_* realizations, one bioim_osim
    realize) between steps gives the same bits, and the env's cache flag is
    still set after the query."""
    from bioimitation import envs
    runs = []
    for query in (True, False):
        random.seed(5)
        env = envs.make(M2D)
        trace = [np.array(env.reset())]
        rng = np.random.default_rng(3)
        T = 8
        for t in range(T):
            o, r, d, info = env.step(rng.uniform(0.0, 1.0, size=env._env.action_dim))
            trace.append(np.concatenate([np.asarray(o, dtype=np.float64), [r, float(d)], info['all_rewards']]))
            if query and t < T - 1:
                assert env.get_state_dict() is not None
                assert (_flags(env._env) == 1).all()
        trace.append(env._env.state_rows().cpu().numpy()[0])
        runs.append(trace)
        env.close()
    for t, (x, y) in enumerate(zip(*runs)):
        assert np.array_equal(x, y), (t, float(np.abs(x - y).max()))


def test_debug_plane_refuses_bad_arguments():
    """bioim_debug_plane with a live handle: an unknown name, a null buffer
    and a wrong size return BIOIM_E_ARG; a plane written and read back is
    what was written, and a write moves nothing else."""
    import ctypes as C
    from bioimitation.vector_env import VectorEnv
    env = VectorEnv(T2D, N, precision=64, seed=2)
    env.reset()
    L, h = env._L, env._h
    buf = np.zeros(N, np.int32)
    vp = buf.ctypes.data_as(C.c_void_p)
    assert L.bioim_debug_plane(h, b'nope', vp, buf.nbytes, 0) == -1 and b"no plane named 'nope'" in L.bioim_last_error()
    assert L.bioim_debug_plane(h, b'cache_ok', None, buf.nbytes, 0) == -1
    assert L.bioim_debug_plane(h, None, vp, buf.nbytes, 0) == -1
    for nbytes in (0, buf.nbytes - 4, buf.nbytes + 4, 2 * buf.nbytes):
        assert L.bioim_debug_plane(h, b'cache_ok', vp, nbytes, 0) == -1
        assert b'holds 128 bytes' in L.bioim_last_error()
        assert L.bioim_debug_plane(h, b'cache_ok', vp, nbytes, 1) == -1
    with pytest.raises(ValueError, match='no state plane'):
        env.debug_plane('nope')
    with pytest.raises(ValueError, match='has shape'):
        env.debug_plane('cache_ok', np.zeros((1, N + 1), np.int32))
    before = env.state_rows().clone()
    r = env.debug_plane('resets')
    assert (r == 1).all()
    env.debug_plane('resets', r + 6)
    assert (env.debug_plane('resets') == 7).all() and env.reset_count() == 7 * N
    import torch
    assert torch.equal(env.state_rows(), before)
    env.close()
