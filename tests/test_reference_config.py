"""config['reference'] in registry.load_pack (no device): a run-time reference
motion replaces the pack's tables as modelpack.compile_pack writes them, and
the episode follows the recipe's own rule."""
import os

import numpy as np
import pytest

import bioimitation
from bioimitation import packdef as P
from bioimitation.modelpack import pack_bytes
from bioimitation.registry import RECIPES, load_pack

DATA = os.path.join(os.path.dirname(bioimitation.__file__), 'data')
W2D, R2D, R3D = 'MuscleWalkingImitation2D-v0', 'MuscleRunningImitation2D-v0', 'MuscleRunningImitation3D-v0'


def _clip(env_id, rows=100, seed=0):
    pk = load_pack(env_id)
    rng = np.random.default_rng(seed)
    return dict(time=0.01 * np.arange(rows), q=rng.normal(size=(rows, pk.ncoord)), u=rng.normal(size=(rows, pk.ncoord)),
                x=rng.normal(size=(rows, P.NREFBODY, 3)))


@pytest.mark.parametrize('env_id', sorted(RECIPES))
def test_the_recipes_own_tables_give_the_committed_pack(env_id):
    """The committed packs were made from the package's data directories by
    the same reader: giving a pack its own directory changes no byte."""
    assert len(RECIPES) == 13
    base = pack_bytes(load_pack(env_id))
    assert pack_bytes(load_pack(env_id, {})) == base
    assert pack_bytes(load_pack(env_id, {'reference': os.path.join(DATA, RECIPES[env_id]['reference'])})) == base
    pk = load_pack(env_id, {'cycle': 7})                              # the cycle override works on its own too
    assert pk.cycle == 7 and pack_bytes(pk) != base
    pk.cycle = load_pack(env_id).cycle
    assert pack_bytes(pk) == base


def test_tables_and_episode():
    ref = _clip(R2D)
    base, pk = load_pack(R2D), load_pack(R2D, {'reference': ref})
    assert (pk.nrows, pk.n_episode, pk.reset_hi, pk.cycle) == (100, 98, 49, base.cycle)     # 'rows-2', 'N/2'
    nc = pk.ncoord
    assert np.array_equal(np.ctypeslib.as_array(pk.ref_q)[:100, :nc], ref['q'])
    assert np.array_equal(np.ctypeslib.as_array(pk.ref_u)[:100, :nc], ref['u'])
    assert np.array_equal(np.ctypeslib.as_array(pk.ref_x)[:100], ref['x'])
    assert np.array_equal(np.array(pk.ref_time[:100]), ref['time'])
    assert list(pk.ref_istep[:100]) == [int(float(t) / 0.01) for t in ref['time']]           # compile_pack's truncation
    for f in ('ref_q', 'ref_u', 'ref_x', 'ref_time', 'ref_istep'):                           # rows past nrows are zero
        a = np.ctypeslib.as_array(getattr(pk, f))
        assert not a[100:].any(), f
        assert f not in ('ref_q', 'ref_u') or not a[:, nc:].any(), f
    # nothing but the reference and the episode changed
    for f in ('nrows', 'n_episode', 'reset_hi'):
        setattr(pk, f, getattr(base, f))
    for f in ('ref_q', 'ref_u', 'ref_x', 'ref_time', 'ref_istep'):
        np.ctypeslib.as_array(getattr(pk, f))[...] = np.ctypeslib.as_array(getattr(base, f))
    assert pack_bytes(pk) == pack_bytes(base)
    # integers of the recipe are capped: Walking2D has N = 264, reset_hi = 132
    pk = load_pack(W2D, {'reference': _clip(W2D)})
    assert (pk.nrows, pk.n_episode, pk.reset_hi, pk.cycle) == (100, 98, 98, 132)
    pk = load_pack(W2D, {'reference': _clip(W2D, 400)})
    assert (pk.nrows, pk.n_episode, pk.reset_hi) == (400, 264, 132)
    pk = load_pack(R3D, {'reference': _clip(R3D, 3)})
    assert (pk.nrows, pk.n_episode, pk.reset_hi) == (3, 1, 0)
    assert load_pack(R3D, {'reference': _clip(R3D, 512)}).nrows == 512


def test_cycle_and_test_mode():
    ref = _clip(W2D)
    assert load_pack(W2D, {'reference': ref, 'cycle': 40}).cycle == 40
    assert load_pack(W2D, {'reference': ref, 'cycle': np.int64(1)}).cycle == 1
    pk = load_pack(W2D, {'reference': ref, 'cycle': 40, 'mode': 'test'})
    assert (pk.nrows, pk.n_episode, pk.reset_hi, pk.cycle) == (100, 98, 0, 40)
    for bad in (0, -3, 2.5, True, '70'):
        for cfg in ({'reference': ref, 'cycle': bad}, {'cycle': bad}):
            with pytest.raises(ValueError, match=r"config\['cycle'\] must be an integer >= 1"):
                load_pack(W2D, cfg)


def test_reference_forms(tmp_path):
    from bioimitation.obslayout import load_names
    from bioimitation.refmotion import ReferenceMotion
    ref = _clip(R3D, 50)
    want = pack_bytes(load_pack(R3D, {'reference': ref}))
    obj = ReferenceMotion(R3D, ref['time'], ref['q'], ref['u'], ref['x'], load_names(R3D)['coords'])
    assert pack_bytes(load_pack(R3D, {'reference': obj})) == want
    # through the four storages: the same pack up to their 10 decimals
    pk = load_pack(R3D, {'reference': obj.save(str(tmp_path / 'clip'))})
    assert sorted(os.listdir(tmp_path / 'clip')) == ['task_BodyKinematics_pos_global.sto', 'task_Kinematics_q.sto',
                                                     'task_Kinematics_u.sto']
    assert (pk.nrows, pk.n_episode) == (50, 48)
    for f, k in (('ref_q', 'q'), ('ref_u', 'u'), ('ref_x', 'x')):
        a = np.ctypeslib.as_array(getattr(pk, f))[:50]
        assert np.abs(a[:, :ref[k].shape[1]] - ref[k]).max() <= 0.5000001e-10, f


def test_refusals(tmp_path):
    ref = _clip(W2D)

    def refused(msg, **change):
        with pytest.raises(ValueError, match=msg) as e:
            load_pack(W2D, {'reference': {**ref, **change}})
        assert str(e.value).startswith(W2D + ": config['reference']")
    refused('q and u .rows, 9.', q=ref['q'][:, :8])
    refused('time must have shape', u=ref['u'][:99])
    refused('x .rows, 9, 3.', x=ref['x'][:, :8])
    refused('time must have shape', time=ref['time'][:, None])
    refused('must hold real numbers', q=[['a'] * 9] * 100)
    refused('non-finite', q=np.where(np.arange(900).reshape(100, 9) == 17, np.nan, ref['q']))
    refused('non-finite', x=np.full_like(ref['x'], np.inf))
    refused('uniform grid 0, 0.01', time=ref['time'] + 0.2)                     # an env reads row istep
    refused('uniform grid 0, 0.01', time=0.02 * np.arange(100))
    refused('uniform grid 0, 0.01', time=np.where(np.arange(100) == 50, 0.5004, ref['time']))
    for rows in (2, 513):
        with pytest.raises(ValueError, match=f'{rows} rows; a clip may be 3 to 512 rows .*0.02 s to 5.11 s'):
            load_pack(W2D, {'reference': _clip(W2D, rows)})
    with pytest.raises(ValueError, match=r"the dict lacks \['u'\]"):
        load_pack(W2D, {'reference': {k: v for k, v in ref.items() if k != 'u'}})
    with pytest.raises(ValueError, match='is not a directory'):
        load_pack(W2D, {'reference': str(tmp_path / 'nowhere')})
    with pytest.raises(ValueError, match='must be a ReferenceMotion, a dict .* or a directory'):
        load_pack(W2D, {'reference': 3})


def test_mixed_batch_refuses_a_reference():
    """The tables belong to one model: refused before anything touches a device."""
    from bioimitation.vector_env import MixedVectorEnv
    with pytest.raises(ValueError, match="MixedVectorEnv: config\\['reference'\\]"):
        MixedVectorEnv([('MuscleLockedKneeImitation3D-v0', 2), ('MusclePalsyImitation3D-v0', 2)],
                       config={'reference': _clip(W2D)})
