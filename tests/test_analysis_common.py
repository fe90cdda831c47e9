"""bioimitation._analysis: the argument checks and the host-to-device move the
six analysis wrappers share.  No device: torch tensors stay on the CPU."""
import numpy as np
import pytest
import torch

from bioimitation import _analysis as A

NAME = 'some analysis'


def raises(msg, fn, *a, **kw):
    with pytest.raises(ValueError) as e:
        fn(*a, **kw)
    assert str(e.value) == msg, str(e.value)


@pytest.mark.parametrize('dtype, kind', [
    (np.float32, 'f'), (np.float64, 'f'), (np.int64, 'i'), (np.int8, 'i'), (np.uint8, 'u'), (np.bool_, 'b'),
    (np.complex128, 'c'),
    (torch.float32, 'f'), (torch.float64, 'f'), (torch.float16, 'f'), (torch.int64, 'i'), (torch.int32, 'i'),
    (torch.uint8, 'i'), (torch.bool, 'b'), (torch.complex64, 'c')])
def test_dtype_kind(dtype, kind):
    x = torch.zeros(2, dtype=dtype) if isinstance(dtype, torch.dtype) else np.zeros(2, dtype=dtype)
    assert A.dtype_kind(x) == kind


def test_check_shape_accepts_arrays_tensors_and_lists():
    assert A.check_shape(NAME, np.zeros((4, 9)), 'q', (9,)) == (4, 9)
    assert A.check_shape(NAME, torch.zeros(4, 7, 6, dtype=torch.int64), 'ext', (7, 6)) == (4, 7, 6)
    assert A.check_shape(NAME, [[0.0] * 9] * 3, 'q', (9,)) == (3, 9)
    assert A.check_shape(NAME, np.zeros((0, 9)), 'q', (9,)) == (0, 9)
    assert A.check_shape(NAME, [1, 2, 3], 'weights', (3,), batched=False) == (3,)
    assert A.check_shape(NAME, np.zeros((2, 3), dtype=bool), 'cactive', (3,), kinds='fiub') == (2, 3)


def test_check_shape_messages_carry_the_callers_prefix():
    raises('some analysis: q must have shape (n, 9), got (4, 8)', A.check_shape, NAME, np.zeros((4, 8)), 'q', (9,))
    raises('some analysis: q must have shape (n, 9), got (9,)', A.check_shape, NAME, np.zeros(9), 'q', (9,))
    raises('joint reaction: ext must have shape (n, 7, 6), got (4, 7, 5)',
           A.check_shape, 'joint reaction', torch.zeros(4, 7, 5), 'ext', (7, 6))
    raises('some analysis: weights must have shape (5,), got (4,)',
           A.check_shape, NAME, np.zeros(4), 'weights', (5,), batched=False)
    raises('some analysis: weights must have shape (5,), got (2, 5)',
           A.check_shape, NAME, np.zeros((2, 5)), 'weights', (5,), batched=False)
    for x in (np.zeros((4, 9), dtype=bool), np.zeros((4, 9), dtype=complex), torch.zeros(4, 9, dtype=torch.bool),
              torch.zeros(4, 9, dtype=torch.complex64)):
        raises(f'some analysis: q must hold real numbers, got dtype {x.dtype}', A.check_shape, NAME, x, 'q', (9,))
    raises('some analysis: q must hold real numbers, got dtype <U1', A.check_shape, NAME, [['a'] * 9], 'q', (9,))
    raises('some analysis: q must hold real numbers', A.check_shape, NAME, [[1.0, 2.0], [3.0]], 'q', (2,))


def test_check_rows_counts_and_refuses_a_mismatch():
    q, ft = np.zeros((3, 9)), torch.zeros(3, 14)
    assert A.check_rows(NAME, (q, 'q', (9,)), ((None, 'u', (9,)), (ft, 'ft', (14,)))) == 3
    assert A.check_rows(NAME, (q.tolist(), 'q', (9,)), ()) == 3
    assert A.check_rows(NAME, (q, 'q', (9,)), ((np.zeros((3, 2), dtype=bool), 'cactive', (2,), 'fiub'),)) == 3
    raises('some analysis: u has 2 rows, q has 3', A.check_rows, NAME, (q, 'q', (9,)), ((np.zeros((2, 9)), 'u', (9,)),))
    raises('some analysis: q0 has 2 rows, x_exp has 3 frames',
           A.check_rows, NAME, (np.zeros((3, 5, 3)), 'x_exp', (5, 3)), ((np.zeros((2, 9)), 'q0', (9,)),), ' frames')
    raises('some analysis: ft must have shape (n, 14), got (3, 13)',
           A.check_rows, NAME, (q, 'q', (9,)), ((np.zeros((3, 13)), 'ft', (14,)),))
    raises('some analysis: cactive must hold real numbers, got dtype bool',
           A.check_rows, NAME, (q, 'q', (9,)), ((np.zeros((3, 2), dtype=bool), 'cactive', (2,)),))


def test_check_want():
    keys = ('a', 'b', 'c')
    assert A.check_want(NAME, 'b', keys) == ('b',)
    assert A.check_want(NAME, ['c', 'a'], keys) == ('c', 'a')
    assert A.check_want(NAME, keys, keys) == keys
    raises('some analysis: nothing requested (want is empty)', A.check_want, NAME, (), keys)
    raises("some analysis: unknown key 'd'; choose from ('a', 'b', 'c')", A.check_want, NAME, ('a', 'd'), keys)


def test_to_device_and_ptr():
    assert A.to_device(None, 'cpu', torch.float64) is None and A.ptr(None) is None
    ro = np.arange(6, dtype=np.float32).reshape(2, 3)
    ro.flags.writeable = False
    t = A.to_device(ro, 'cpu', torch.float64)
    assert t.dtype == torch.float64 and t.is_contiguous() and t.tolist() == [[0, 1, 2], [3, 4, 5]]
    t[0, 0] = 7.0                        # a copy: the read-only array is not written through
    assert ro[0, 0] == 0
    assert A.to_device([[1, 2], [3, 4]], 'cpu', torch.float32).dtype == torch.float32
    nc = torch.arange(6.0).reshape(2, 3).t()
    c = A.to_device(nc, 'cpu', torch.float64)
    assert c.is_contiguous() and torch.equal(c, nc.double())
    assert A.to_device(np.array([True, False]), 'cpu', torch.uint8).tolist() == [1, 0]
    assert A.ptr(c).value == c.data_ptr()


@pytest.mark.parametrize('module, name', [
    ('muscle_analysis', 'muscle analysis'), ('static_optimization', 'static optimization'),
    ('inverse_kinematics', 'inverse kinematics'), ('joint_reaction', 'joint reaction'),
    ('induced_accelerations', 'induced accelerations')])
def test_the_wrappers_check_want_against_their_own_keys(module, name):
    import importlib
    m = importlib.import_module('bioimitation.' + module)
    assert m.NAME == name
    args = {'muscle_analysis': (9, 14, None), 'static_optimization': (9, 14, None), 'inverse_kinematics': (9, 5, None),
            'joint_reaction': (9, 14, 7, None), 'induced_accelerations': (9, 14, 7, 2, None)}[module]
    raises(f'{name}: nothing requested (want is empty)', m.check_args, *args, want=())
    raises(f"{name}: unknown key 'nope'; choose from {m.KEYS}", m.check_args, *args, want=('nope',))
