"""bioim_rollout / bioim_rollout_fused (include/bioim.h): the header declares
them, the binding lists them, and their argument checks return BIOIM_E_ARG
(-1) with a message before any device call — so all of this runs without a
GPU."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('bioim_rollout', 'bioim_rollout_fused')


def _lib_or_skip():
    from bioimitation import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libbioim.so not built')
    return _lib, _lib.load()


def test_header_declares_the_rollout_calls():
    txt = open(os.path.join(REPO, 'include', 'bioim.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    assert re.search(r'int bioim_rollout\(bioim_handle_t \*h, const void \*actions, int steps, int64_t action_step_stride,\s*'
                     r'void \*obs_seq, void \*obs_last, void \*reward_seq, uint8_t \*done_seq, void \*info_seq,\s*'
                     r'int stop_at_done\);', code)
    assert re.search(r'int bioim_rollout_fused\(const bioim_handle_t \*h\);', code)
    # the comment states the contract, the two paths and the refusals
    doc = txt[txt.index('bioim_rollout: `steps` consecutive'):txt.index('int bioim_rollout(')]
    doc = ' '.join(doc.replace('\n *', ' ').split())
    for word in ('bit for bit', 'stop_at_done', 'ONE launch', 'auto-reset', 'budgeted', 'frame skip',
                 'No reference counterpart'):
        assert word in doc, word


def test_binding_lists_them():
    from bioimitation import _lib
    for n in NAMES:
        assert n in _lib.EXPORTS


def test_null_handle_is_an_argument_error():
    _lib, L = _lib_or_skip()
    p = C.cast(C.create_string_buffer(64), C.c_void_p)
    assert L.bioim_rollout(None, None, 0, 0, None, None, None, None, None, 0) == -1
    assert b'bioim_rollout: null handle' in L.bioim_last_error()
    assert L.bioim_rollout(None, p, 3, 1, p, p, p, p, p, 0) == -1
    assert b'bioim_rollout: null handle' in L.bioim_last_error()
    assert L.bioim_rollout_fused(None) == -1
    assert b'bioim_rollout_fused: null handle' in L.bioim_last_error()


def test_null_buffers_bad_steps_and_stride_are_argument_errors():
    """With a handle: the checks come before any device call.  The handle is
    a zeroed block at least as large as the library's handle (the trick of
    test_state_clone_abi.py): 0 envs, semi-implicit, no budget, auto-reset
    off — so each call below ends in the argument check it is about."""
    _lib, L = _lib_or_skip()
    from bioimitation import packdef
    blk = C.create_string_buffer(C.sizeof(packdef.ModelPack) + 65536)
    h = C.cast(blk, C.c_void_p)
    p = C.cast(C.create_string_buffer(64), C.c_void_p)
    assert L.bioim_rollout(h, None, 2, 0, None, None, p, p, None, 0) == -1
    assert b'bioim_rollout: null actions or done_seq' in L.bioim_last_error()
    assert L.bioim_rollout(h, p, 2, 0, None, None, p, None, None, 0) == -1
    assert b'bioim_rollout: null actions or done_seq' in L.bioim_last_error()
    for steps in (0, -2):
        assert L.bioim_rollout(h, p, steps, 0, None, None, p, p, None, 0) == -1
        assert b'bioim_rollout: steps must be positive' in L.bioim_last_error()
    assert L.bioim_rollout(h, p, 2, -1, None, None, p, p, None, 0) == -1
    assert b'bioim_rollout: negative action_step_stride' in L.bioim_last_error()
    assert L.bioim_rollout_fused(h) == 0      # no rollout ran on it
