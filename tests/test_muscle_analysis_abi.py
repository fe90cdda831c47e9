"""bioim_muscle_eval (include/bioim.h): the header declares it, the binding
lists it, and its argument checks return BIOIM_E_ARG (-1) with a message
before any device call; the ValueError paths of MuscleAnalysis.eval's
argument check need no device either.  All of this runs without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'bioim_muscle_eval'


def _lib_or_skip():
    from bioimitation import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libbioim.so not built')
    return _lib, _lib.load()


def test_header_declares_the_call():
    txt = open(os.path.join(REPO, 'include', 'bioim.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    assert re.search(r'#define BIOIM_MUSCLE_FIBER_DIM 5\b', code)
    assert re.search(r'int bioim_muscle_eval\(bioim_handle_t \*h, int n, const void \*q, const void \*u, '
                     r'const void \*act, const void \*lce,\s*void \*length, void \*speed, void \*dldq, '
                     r'void \*fiber, void \*tau\);', code)
    doc = txt[txt.index('Muscle analysis ('):txt.index('#define BIOIM_MUSCLE_FIBER_DIM')]
    doc = ' '.join(doc.replace('\n *', ' ').split())
    for word in ('exact zeros', 'moment arm is -dL/dq', 'static equilibrium', 'started cold', 'any output may be NULL',
                 'neither read nor written', 'BIOIM_E_ARG', 'synchronizes nothing', 'No reference counterpart'):
        assert word in doc, word


def test_binding_lists_it():
    from bioimitation import _lib
    assert NAME in _lib.EXPORTS
    from bioimitation import muscle_analysis
    assert muscle_analysis.FIBER_DIM == 5


def test_library_exports_it():
    _lib, L = _lib_or_skip()
    assert hasattr(L, NAME)
    assert L.bioim_muscle_eval.argtypes is not None and len(L.bioim_muscle_eval.argtypes) == 11


def test_refusals_come_before_any_device_call():
    """Each refusal of the header, in turn.  The handle is a zeroed block at
    least as large as the library's handle (the trick of
    test_rollout_abi.py): its model has no muscles, which is the last check,
    so every call below ends in the argument check it is about."""
    _lib, L = _lib_or_skip()
    from bioimitation import packdef
    blk = C.create_string_buffer(C.sizeof(packdef.ModelPack) + 65536)
    h = C.cast(blk, C.c_void_p)
    p = C.cast(C.create_string_buffer(64), C.c_void_p)

    def refused(msg, *args):
        assert L.bioim_muscle_eval(*args) == -1, msg
        err = L.bioim_last_error()
        assert err.startswith(b'bioim_muscle_eval:') and msg in err, (msg, err)
    refused(b'null handle', None, 1, p, p, p, p, p, p, p, p, p)
    refused(b'null handle', None, 0, None, None, None, None, None, None, None, None, None)
    refused(b'negative n', h, -1, p, p, p, p, p, p, p, p, p)
    refused(b'null q', h, 1, None, p, p, p, p, p, p, p, p)
    refused(b'no output requested', h, 1, p, p, p, p, None, None, None, None, None)
    refused(b'no output requested', h, 0, None, None, None, None, None, None, None, None, None)
    refused(b'fiber and tau need act', h, 1, p, p, None, p, p, p, p, p, None)     # fiber without act
    refused(b'fiber and tau need act', h, 1, p, p, None, None, None, None, None, None, p)   # tau without act
    refused(b'the model has no muscles', h, 1, p, p, p, p, p, p, p, p, p)
    refused(b'the model has no muscles', h, 1, p, None, None, None, p, None, None, None, None)
    refused(b'the model has no muscles', h, 0, None, None, None, None, p, None, None, None, None)


def test_eval_argument_errors_need_no_device():
    """MuscleAnalysis.eval checks its arguments with check_args before the
    library call: shapes, dtypes, unknown keys, missing inputs."""
    from bioimitation.muscle_analysis import DEFAULT_WANT, KEYS, check_args
    nd, nm, n = 9, 14, 3
    q, u = np.zeros((n, nd)), np.zeros((n, nd))
    act, lce = np.full((n, nm), 0.5), np.full((n, nm), 0.1)
    assert check_args(nd, nm, q) == (n, DEFAULT_WANT)
    assert check_args(nd, nm, q, u, act, lce, KEYS) == (n, KEYS)
    assert check_args(nd, nm, q.tolist(), want='length') == (n, ('length',))
    assert check_args(nd, nm, q, act=act, want=('fiber', 'tau')) == (n, ('fiber', 'tau'))
    assert check_args(nd, nm, np.zeros((0, nd)))[0] == 0
    bad = [
        (dict(q=None), 'q is required'),
        (dict(q=np.zeros(nd)), 'shape'),
        (dict(q=np.zeros((n, nd + 1))), 'shape'),
        (dict(q=np.zeros((n, 1, nd))), 'shape'),
        (dict(q=q, u=np.zeros((n, nm))), 'u must have shape'),
        (dict(q=q, u=np.zeros((n + 1, nd))), 'rows'),
        (dict(q=q, act=np.zeros((n, nd))), 'act must have shape'),
        (dict(q=q, act=act, lce=np.zeros((n - 1, nm))), 'rows'),
        (dict(q=q, act=act, lce=np.zeros(nm)), 'lce must have shape'),
        (dict(q=q.astype(complex)), 'real numbers'),
        (dict(q=q, u=np.zeros((n, nd), dtype=bool)), 'real numbers'),
        (dict(q=q, act=np.full((n, nm), 'a')), 'real numbers'),
        (dict(q=q, want=('length', 'force')), 'unknown key'),
        (dict(q=q, want=()), 'nothing requested'),
        (dict(q=q, want=('fiber',)), 'needs the activations'),
        (dict(q=q, lce=lce, want=('tau',)), 'needs the activations'),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            check_args(nd, nm, **kw)


def test_eval_checks_torch_tensors_too():
    torch = pytest.importorskip('torch')
    from bioimitation.muscle_analysis import check_args
    q = torch.zeros((2, 9), dtype=torch.float32)
    assert check_args(9, 14, q, act=torch.zeros((2, 14), dtype=torch.float64), want=('tau',))[0] == 2
    with pytest.raises(ValueError, match='real numbers'):
        check_args(9, 14, q, u=torch.zeros((2, 9), dtype=torch.bool))
    with pytest.raises(ValueError, match='real numbers'):
        check_args(9, 14, torch.zeros((2, 9), dtype=torch.complex64))
    with pytest.raises(ValueError, match='shape'):
        check_args(9, 14, torch.zeros(9))
