"""Device-side indexed state save / restore and env cloning:
``VectorEnv.state_rows(env_ids=...)``, ``load_state`` and ``clone_envs`` over
bioim_copy_state_rows / bioim_load_state / bioim_clone_envs.

Every comparison is bitwise.  35 envs at 16 envs per workgroup are two full
workgroups and a partial one; the clone's source (1) and targets (0, 17, 33,
34) sit in different workgroups, in the partial one, and — 0 and 1 — in the
two envs that share a 32-lane group."""
import ctypes as C

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason='needs a HIP GPU')]

N = 35
WARM = 6            # steps before the clone: caches valid, fiber-velocity warm starts warm
SRC, DST = 1, [0, 17, 33, 34]
M2D = 'MuscleWalkingImitation2D-v0'


def _rows(pk):
    """a distinct reference row per env"""
    assert pk.reset_hi + 1 >= N
    return np.random.default_rng(11).permutation(pk.reset_hi + 1)[:N].astype(np.int32)


def _actions(pk, rows, T, seed=12):
    """muscle models U[0, 0.3]; torque models the reference targets of the
    next row + N(0, 0.02) (the golden perturbation cases' actions)"""
    rng = np.random.default_rng(seed)
    if pk.nmuscle:
        return rng.uniform(0.0, 0.3, size=(T, N, pk.nact))
    return np.stack([np.array([[pk.ref_q[min(int(r) + t + 1, pk.nrows - 1)][pk.pd_coord[a]] for a in range(pk.nact)]
                               for r in rows]) for t in range(T)]) + rng.normal(0.0, 0.02, size=(T, N, pk.nact))


def _make(env_id, rows, precision=64, config=None):
    from bioimitation.vector_env import VectorEnv
    env = VectorEnv(env_id, N, config=config, precision=precision, auto_reset=False)
    assert env.launch['envs_per_workgroup'] == 16
    env.reset(ref_index=rows)
    return env


def _act(env, a):
    import torch
    return torch.as_tensor(a, device=env.device, dtype=env.dtype)


def _setup(env_id, T, precision=64, count=1, config=None):
    from bioimitation.registry import load_pack
    pk = load_pack(env_id)
    rows = _rows(pk)
    acts = _actions(pk, rows, T)
    envs = [_make(env_id, rows, precision, config) for _ in range(count)]
    for t in range(WARM):
        for e in envs:
            e.step(_act(e, acts[t]))
    return envs, acts


def _outputs(env):
    """the step's output rows and the flat state rows, as one tuple of (N, ...) tensors"""
    return env.obs, env.reward, env.done, env.info, env.state_rows()


def _rows_equal(xs, i, ys, j):
    import torch
    return all(torch.equal(x[i], y[j]) for x, y in zip(xs, ys))


def _clone_continues(env_id, precision, steps_after):
    import torch
    (a, b), acts = _setup(env_id, WARM + steps_after, precision, count=2)
    before = a.state_rows()
    for d in DST:
        assert not torch.equal(before[d], before[SRC]), d
    resets = a.reset_count()
    a.clone_envs(SRC, DST)
    assert a.reset_count() == resets
    after = a.state_rows()
    for d in DST:
        assert torch.equal(after[d], after[SRC]), d
    untouched = [i for i in range(N) if i not in DST]
    for t in range(WARM, WARM + steps_after):
        act = acts[t].copy()
        act[DST] = act[SRC]
        a.step(_act(a, act))
        b.step(_act(b, acts[t]))
        oa, ob = _outputs(a), _outputs(b)
        for d in DST:
            assert _rows_equal(oa, d, oa, SRC), (env_id, precision, t, d)
        assert _rows_equal(oa, untouched, ob, untouched), (env_id, precision, t)
    assert a.reset_count() == resets
    a.close()
    b.close()


def test_clone_continues_bit_for_bit():
    """Env 1 cloned into 0, 17, 33 and 34 after 6 steps: under the source's
    actions every clone's obs, reward, done, info and state rows equal the
    source's for 8 more steps; the other envs equal an un-cloned run's; the
    reset count does not move."""
    _clone_continues(M2D, 64, 8)


@pytest.mark.parametrize('env_id,precision', [('TorqueWalkingImitation2D-v0', 64), ('MuscleRunningImitation3D-v0', 64),
                                              (M2D, 32)])
def test_clone_other_kernels_and_precisions(env_id, precision):
    _clone_continues(env_id, precision, 3)


def test_clone_carries_what_the_flat_row_lacks():
    """One target cloned, another given the source's flat row by load_state:
    after the next step the clone equals the source bitwise and the loaded
    env differs from it somewhere (its first substep had no realize cache:
    the cache row really travelled with the clone).

    The source must be an env whose next step depends on its cache row at
    all, and most do not: measured on an MI355X with this file's setup, a
    dropped cache changed the next observation of 1 env in 35 (env 5 at step
    6; env 1, the source of the other tests, in none of steps 6..11; max
    relative change 3.3e-13).  So the source is not fixed: a twin batch whose
    caches the host path drops (set_state, as test_realize_cache_first_substep
    does) shows, step by step, which envs' next step the cache changes, and
    the first such env is cloned."""
    import torch
    (a, ref, probe), acts = _setup(M2D, WARM + 8, count=3)
    src = None
    for t in range(WARM, WARM + 8):
        probe.set_state(ref.get_state())        # ref's flat state, no cache rows
        act = _act(ref, acts[t])
        differs = (ref.step(act)[0] != probe.step(act)[0]).any(dim=1).cpu().numpy()
        if differs.any():
            src = int(np.nonzero(differs)[0][0])
            break
        a.step(act)                             # a follows ref, one step behind the probe
    assert src is not None, 'no env whose next step the realize cache changes: the test shows nothing'
    dst, dst2 = [i for i in (17, 33, 0) if i != src][:2]
    a.clone_envs(src, [dst])
    a.load_state(a.state_rows(env_ids=[src]), [dst2])
    s = a.state_rows()
    assert torch.equal(s[dst], s[src]) and torch.equal(s[dst2], s[src])
    act = acts[t].copy()
    act[[dst, dst2]] = act[src]
    obs = a.step(_act(a, act))[0]
    assert torch.equal(obs[src], ref.obs[src])
    assert torch.equal(obs[dst], obs[src])
    assert bool((obs[dst2] != obs[src]).any()), 'the loaded env equals the source bitwise: the cache was never used'
    for e in (a, ref, probe):
        e.close()


def test_load_equals_host_path_and_touches_only_listed():
    """A: get_state / set_state with rows src copied over dst on the host.
    B: load_state(state_rows(env_ids=src), dst).  C: nothing.  B's dst rows
    equal A's; B's other rows equal C's — which A's do not, set_state having
    cleared every env's realize cache."""
    (a, b, c), acts = _setup(M2D, WARM + 5, count=3)
    src, dst = [1, 20], [0, 34]
    s = a.get_state()
    s[dst] = s[src]
    a.set_state(s)
    b.load_state(b.state_rows(env_ids=src), dst)
    others = [i for i in range(N) if i not in dst]
    a_differs = False
    for t in range(WARM, WARM + 5):
        act = acts[t].copy()
        act[dst] = act[src]
        for e in (a, b, c):
            e.step(_act(e, act))
        oa, ob, oc = _outputs(a), _outputs(b), _outputs(c)
        assert _rows_equal(ob, dst, oa, dst), t
        assert _rows_equal(ob, others, oc, others), t
        a_differs = a_differs or not _rows_equal(oa, others, oc, others)
    assert a_differs, 'the host path left the other envs bit-equal too: the check above shows nothing'
    for e in (a, b, c):
        e.close()


def test_clone_of_a_suspended_rk_step_resumes_identically():
    """RK-Merson with a budget of 2 attempts per launch: an env suspended
    mid-step is cloned; the clones' ready flags and state rows equal the
    source's at every launch, and their output rows whenever a step finishes,
    until the source has finished two env steps."""
    import torch
    from bioimitation.registry import load_pack
    from bioimitation.vector_env import VectorEnv
    pk = load_pack(M2D)
    rows = _rows(pk)
    T = 20
    acts = _actions(pk, rows, T)
    env = VectorEnv(M2D, N, config={'integrator': 'rk-merson'}, precision=64, auto_reset=False)
    env.set_rk_budget(2)
    env.reset(ref_index=rows)
    k = 0
    while k < 4 and (k == 0 or env.pending_count() == 0):
        env.step(_act(env, acts[k]))
        k += 1
    assert env.pending_count() > 0, 'no env was suspended: the test does not exercise the resume path'
    ready = env.ready.cpu().numpy()
    src = int(np.nonzero(ready == 0)[0][0])
    dst = [i for i in (0, 17, 34, 33) if i != src][:3]
    env.clone_envs(src, dst)
    finished = 0
    while finished < 2 and k < T:
        act = acts[k].copy()
        act[dst] = act[src]
        env.step(_act(env, act))
        k += 1
        ready, s = env.ready, env.state_rows()
        out = (env.obs, env.reward, env.done, env.info)
        fin = bool(ready[src])
        for d in dst:
            assert bool(ready[d]) == fin, (k, d)
            assert torch.equal(s[d], s[src]), (k, d)
            if fin:
                assert _rows_equal(out, d, out, src), (k, d)
        finished += fin
    assert finished == 2, (finished, k)
    env.close()


def test_subset_gather():
    import torch
    (a,), _ = _setup(M2D, WARM)
    want = torch.from_numpy(a.get_state()[[34, 0, 16]])
    assert torch.equal(a.state_rows(env_ids=[34, 0, 16]).cpu(), want)
    assert torch.equal(a.state_rows(env_ids=np.array([34, 0, 16])).cpu(), want)
    ids = torch.tensor([34, 0, 16], device=a.device)
    out = torch.zeros((3, a.state_dim), dtype=torch.float64, device=a.device)
    assert a.state_rows(out=out, env_ids=ids) is out
    assert torch.equal(out.cpu(), want)
    assert torch.equal(a.state_rows().cpu(), torch.from_numpy(a.get_state()))
    a.close()


def test_id_forms_and_load_all():
    """src as a list with repeats, ids as numpy arrays and device tensors;
    load_state without ids restores every env."""
    import torch
    (a, b), acts = _setup('TorqueWalkingImitation2D-v0', WARM + 2, count=2)
    saved = a.state_rows()
    a.clone_envs([1, 1, 20], np.array([0, 34, 17]))
    a.clone_envs(torch.tensor([2, 2], device=a.device), torch.tensor([33, 16], device=a.device))
    s = a.state_rows()
    for d, src in ((0, 1), (34, 1), (17, 20), (33, 2), (16, 2)):
        assert torch.equal(s[d], s[src])
    a.load_state(saved)
    assert torch.equal(a.state_rows(), saved)
    for t in range(WARM, WARM + 2):
        a.step(_act(a, acts[t]))
        b.step(_act(b, acts[t]))
        assert _rows_equal(_outputs(a), slice(None), _outputs(b), slice(None)), t
    a.close()
    b.close()


def test_validation_refuses_on_the_host():
    """Bad ids and buffers raise ValueError in the Python layer, before any
    launch: the state is unchanged afterwards.  The C entry points' own
    argument errors (null buffers, n out of range — never a bad id) return
    BIOIM_E_ARG."""
    import torch
    (a,), _ = _setup(M2D, WARM)
    before = a.state_rows().clone()
    good = a.state_rows(env_ids=[1])
    for bad in (35, -1):
        with pytest.raises(ValueError, match=r'lie in \[0, 35\)'):
            a.clone_envs(1, [0, bad])
        with pytest.raises(ValueError, match=r'lie in \[0, 35\)'):
            a.clone_envs(bad, [0, 2])
        with pytest.raises(ValueError, match=r'lie in \[0, 35\)'):
            a.load_state(good, [bad])
        with pytest.raises(ValueError, match=r'lie in \[0, 35\)'):
            a.state_rows(env_ids=[0, bad])
        with pytest.raises(ValueError, match=r'lie in \[0, 35\)'):
            a.clone_envs(1, torch.tensor([0, bad], device=a.device))
    with pytest.raises(ValueError, match='distinct'):
        a.clone_envs(1, [0, 17, 0])
    with pytest.raises(ValueError, match='distinct'):
        a.load_state(a.state_rows(env_ids=[1, 1]), [3, 3])
    with pytest.raises(ValueError, match='both a src and a dst'):
        a.clone_envs([1, 0], [0, 17])
    with pytest.raises(ValueError, match='both a src and a dst'):
        a.clone_envs(17, [0, 17])
    with pytest.raises(ValueError, match='src ids for'):
        a.clone_envs([1, 2, 3], [0, 17])
    with pytest.raises(ValueError, match='integers'):
        a.clone_envs(1, [0.5, 2.0])
    two = a.state_rows(env_ids=[1, 2])
    for rows in (two.float(), two[:1], two[:, :-1].contiguous(), two.cpu(),
                 torch.zeros((2, 2 * a.state_dim), dtype=torch.float64, device=a.device)[:, ::2], two.cpu().numpy()):
        with pytest.raises(ValueError, match='load_state: rows must be a contiguous'):
            a.load_state(rows, [3, 4])
    with pytest.raises(ValueError, match='load_state: rows'):
        a.load_state(two)                      # 2 rows for all 35 envs
    for out in (torch.zeros((N, a.state_dim), dtype=torch.float32, device=a.device),
                torch.zeros((N - 1, a.state_dim), dtype=torch.float64, device=a.device),
                torch.zeros((N, a.state_dim), dtype=torch.float64),                                   # on the host
                torch.zeros((N, a.state_dim + 1), dtype=torch.float64, device=a.device)[:, :-1],      # row stride
                torch.zeros((N, 2 * a.state_dim), dtype=torch.float64, device=a.device)[:, ::2],      # not contiguous
                torch.zeros((a.state_dim, N), dtype=torch.float64, device=a.device),                  # transposed shape
                np.zeros((N, a.state_dim))):
        with pytest.raises(ValueError, match='state_rows: out must be a contiguous'):
            a.state_rows(out=out)
    with pytest.raises(ValueError, match='state_rows: out'):
        a.state_rows(out=torch.zeros((N, a.state_dim), dtype=torch.float64, device=a.device), env_ids=[1, 2])
    L, h, p = a._L, a._h, a._ptr
    ids = torch.tensor([0, 1], dtype=torch.int32, device=a.device)
    assert L.bioim_copy_state_rows(h, p(ids), 2, None) == -1 and L.bioim_load_state(h, p(ids), 2, None) == -1
    assert L.bioim_clone_envs(h, None, p(ids), 2) == -1 and L.bioim_clone_envs(h, p(ids), None, 2) == -1
    for n in (0, -1, N + 1):
        assert L.bioim_copy_state_rows(h, p(ids), n, p(two)) == -1
        assert L.bioim_load_state(h, p(ids), n, p(two)) == -1
        assert L.bioim_clone_envs(h, p(ids), p(ids), n) == -1
        assert b'n must lie in' in L.bioim_last_error()
    assert torch.equal(a.state_rows(), before)
    a.close()
