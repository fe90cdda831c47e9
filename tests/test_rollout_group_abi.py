"""bioim_rollout_group / bioim_rollout_group_fused (include/bioim.h): the
header declares them, the binding lists them, and their argument checks
return BIOIM_E_ARG (-1) with a message starting ``bioim_rollout_group:``
before any device call — so all of this runs without a GPU."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('bioim_rollout_group', 'bioim_rollout_group_fused')


def _lib_or_skip():
    from bioimitation import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libbioim.so not built')
    return _lib, _lib.load()


def test_header_declares_the_group_rollout_calls():
    txt = open(os.path.join(REPO, 'include', 'bioim.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    assert re.search(r'int bioim_rollout_group\(bioim_handle_t \*\*hs, int nh, const void \*actions, int steps, '
                     r'int64_t action_step_stride,\s*void \*obs_seq, void \*obs_last, void \*reward_seq, '
                     r'uint8_t \*done_seq, void \*info_seq,\s*int stop_at_done\);', code)
    assert re.search(r'int bioim_rollout_group_fused\(const bioim_handle_t \*h\);', code)
    # the comment states the contract, the two paths and the refusals
    doc = txt[txt.index('bioim_rollout_group: `steps` consecutive'):txt.index('int bioim_rollout_group(')]
    doc = ' '.join(doc.replace('\n *', ' ').split())
    for word in ('bit for bit', 'stop_at_done', 'ONE launch', 'auto-reset', 'budgeted', 'No reference counterpart'):
        assert word in doc, word


def test_binding_lists_them():
    from bioimitation import _lib
    for n in NAMES:
        assert n in _lib.EXPORTS


def _zeroed_handle():
    """a zeroed block at least as large as the library's handle (the trick of
    test_rollout_abi.py): 0 envs, device 0, precision 0, strides 0,
    semi-implicit, no budget, auto-reset off"""
    from bioimitation import packdef
    blk = C.create_string_buffer(C.sizeof(packdef.ModelPack) + 65536)
    return blk, C.cast(blk, C.c_void_p)


def test_null_list_and_null_handles_are_argument_errors():
    _lib, L = _lib_or_skip()
    p = C.cast(C.create_string_buffer(64), C.c_void_p)
    blk, h = _zeroed_handle()
    assert L.bioim_rollout_group(None, 2, p, 3, 1, p, p, p, p, p, 0) == -1
    assert L.bioim_last_error().startswith(b'bioim_rollout_group: null handle list or nh <= 0')
    for nh in (0, -1):
        hs = (C.c_void_p * 2)(h.value, h.value)
        assert L.bioim_rollout_group(hs, nh, p, 3, 1, p, p, p, p, p, 0) == -1
        assert L.bioim_last_error().startswith(b'bioim_rollout_group: null handle list or nh <= 0')
    for hs in ((C.c_void_p * 2)(None, h.value), (C.c_void_p * 2)(h.value, None)):
        assert L.bioim_rollout_group(hs, 2, p, 3, 1, p, p, p, p, p, 0) == -1
        assert L.bioim_last_error().startswith(b'bioim_rollout_group: null handle')
    assert L.bioim_rollout_group_fused(None) == -1
    assert b'bioim_rollout_group_fused: null handle' in L.bioim_last_error()
    assert L.bioim_rollout_group_fused(h) == 0      # no group rollout ran on it


@pytest.mark.parametrize('nh', [1, 2])
def test_null_buffers_bad_steps_and_stride_are_argument_errors(nh):
    """each call ends in the argument check it is about, before any device
    call; with one handle too (the group's own checks come before it hands
    the call to bioim_rollout)"""
    _lib, L = _lib_or_skip()
    p = C.cast(C.create_string_buffer(64), C.c_void_p)
    blk0, h0 = _zeroed_handle()
    blk1, h1 = _zeroed_handle()
    hs = (C.c_void_p * 2)(h0.value, h1.value)
    assert L.bioim_rollout_group(hs, nh, None, 2, 0, None, None, p, p, None, 0) == -1
    assert L.bioim_last_error().startswith(b'bioim_rollout_group: null actions or done_seq')
    assert L.bioim_rollout_group(hs, nh, p, 2, 0, None, None, p, None, None, 0) == -1
    assert L.bioim_last_error().startswith(b'bioim_rollout_group: null actions or done_seq')
    for steps in (0, -2):
        assert L.bioim_rollout_group(hs, nh, p, steps, 0, None, None, p, p, None, 0) == -1
        assert L.bioim_last_error().startswith(b'bioim_rollout_group: steps must be positive')
    assert L.bioim_rollout_group(hs, nh, p, 2, -1, None, None, p, p, None, 0) == -1
    assert L.bioim_last_error().startswith(b'bioim_rollout_group: negative action_step_stride')
    assert L.bioim_rollout_group_fused(h0) == 0


def test_differing_handles_and_stop_at_done_with_auto_reset_are_refused():
    """The handle starts with its int fields `n, device, precision, ndof,
    nmuscle, nact, horizon, obs_dim, info_dim, nsub, auto_reset, env_offset,
    act_stride, obs_stride, info_stride` (struct bioim_handle,
    csrc/bioim_step.hip); the zeroed blocks get the one field each case is
    about.  (A budgeted RK handle and suspended envs need a real handle: the
    GPU tests refuse those.)"""
    _lib, L = _lib_or_skip()
    p = C.cast(C.create_string_buffer(64), C.c_void_p)
    DEVICE, PRECISION, AUTO_RESET, ACT_STRIDE, OBS_STRIDE, INFO_STRIDE = 1, 2, 10, 12, 13, 14
    for field in (DEVICE, PRECISION, ACT_STRIDE, OBS_STRIDE, INFO_STRIDE):
        blk0, h0 = _zeroed_handle()
        blk1, h1 = _zeroed_handle()
        C.cast(blk1, C.POINTER(C.c_int))[field] = 3
        hs = (C.c_void_p * 2)(h0.value, h1.value)
        assert L.bioim_rollout_group(hs, 2, p, 2, 0, None, None, p, p, None, 0) == -1
        assert L.bioim_last_error().startswith(b'bioim_rollout_group: handles differ in device, precision or I/O strides')
    blk0, h0 = _zeroed_handle()
    blk1, h1 = _zeroed_handle()
    C.cast(blk1, C.POINTER(C.c_int))[AUTO_RESET] = 1
    hs = (C.c_void_p * 2)(h0.value, h1.value)
    assert L.bioim_rollout_group(hs, 2, p, 2, 0, None, None, p, p, None, 1) == -1
    assert L.bioim_last_error().startswith(b'bioim_rollout_group: stop_at_done needs auto-reset off')
