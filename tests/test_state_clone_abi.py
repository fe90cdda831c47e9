"""bioim_copy_state_rows / bioim_load_state / bioim_clone_envs (include/bioim.h):
the header declares them, the binding lists them, and their argument checks
return BIOIM_E_ARG (-1) with a message before any device call — so all of
this runs without a GPU."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('bioim_copy_state_rows', 'bioim_load_state', 'bioim_clone_envs')


def _lib_or_skip():
    from bioimitation import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libbioim.so not built')
    return _lib, _lib.load()


def test_header_declares_the_indexed_state_calls():
    txt = open(os.path.join(REPO, 'include', 'bioim.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    assert re.search(r'int bioim_copy_state_rows\(bioim_handle_t \*h, const int32_t \*env_ids, int n, void \*device_out\);', code)
    assert re.search(r'int bioim_load_state\(bioim_handle_t \*h, const int32_t \*env_ids, int n, const void \*device_rows\);', code)
    assert re.search(r'int bioim_clone_envs\(bioim_handle_t \*h, const int32_t \*src_ids, const int32_t \*dst_ids, int n\);', code)
    # the comment of bioim_clone_envs says what stays behind and what a suspended clone does
    doc = txt[txt.index('bioim_clone_envs: for each'):txt.index('int bioim_clone_envs(')]
    for word in ('reset counter', 'suspended', 'draws its own'):
        assert word in doc, word


def test_binding_lists_them():
    from bioimitation import _lib
    for n in NAMES:
        assert n in _lib.EXPORTS


def test_null_handle_is_an_argument_error():
    _lib, L = _lib_or_skip()
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)
    assert L.bioim_copy_state_rows(None, None, 0, None) == -1
    assert b'bioim_copy_state_rows: null handle' in L.bioim_last_error()
    assert L.bioim_copy_state_rows(None, p, 1, p) == -1
    assert L.bioim_load_state(None, None, 0, None) == -1
    assert b'bioim_load_state: null handle' in L.bioim_last_error()
    assert L.bioim_load_state(None, p, 1, p) == -1
    assert L.bioim_clone_envs(None, None, None, 0) == -1
    assert b'bioim_clone_envs: null handle' in L.bioim_last_error()
    assert L.bioim_clone_envs(None, p, p, 1) == -1


def test_null_buffers_and_bad_n_are_argument_errors():
    """With a handle: the checks come before any device call.  The handle here
    is a zeroed block at least as large as the library's handle (which embeds
    the ModelPack), i.e. one of 0 envs: every n > 0 is then too large, so
    each call below ends in an argument check and never reaches the device."""
    _lib, L = _lib_or_skip()
    from bioimitation import packdef
    blk = C.create_string_buffer(C.sizeof(packdef.ModelPack) + 65536)
    h = C.cast(blk, C.c_void_p)
    ids = (C.c_int32 * 4)(0, 1, 2, 3)
    idp = C.cast(ids, C.c_void_p)
    buf = C.cast(C.create_string_buffer(64), C.c_void_p)
    assert L.bioim_copy_state_rows(h, idp, 1, None) == -1
    assert b'null output buffer' in L.bioim_last_error()
    assert L.bioim_load_state(h, idp, 1, None) == -1
    assert b'null rows buffer' in L.bioim_last_error()
    assert L.bioim_clone_envs(h, None, idp, 1) == -1
    assert b'null src or dst' in L.bioim_last_error()
    assert L.bioim_clone_envs(h, idp, None, 1) == -1
    assert b'null src or dst' in L.bioim_last_error()
    # bioim_debug_plane (debug / tests): the name, the buffer and the size are checked first
    dbg = L.bioim_debug_plane
    assert dbg(None, b'cache_ok', buf, 0, 0) == -1
    assert b'bioim_debug_plane: null handle' in L.bioim_last_error()
    assert dbg(h, None, buf, 0, 0) == -1 and dbg(h, b'cache_ok', None, 0, 0) == -1
    assert b'null plane name or host buffer' in L.bioim_last_error()
    for write in (0, 1):
        assert dbg(h, b'cache_okay', buf, 0, write) == -1
        assert b"no plane named 'cache_okay'" in L.bioim_last_error()
        for name in (b'cache', b'cache_ok', b'vnw', b'ctl', b'pend', b'resets', b'rkev'):
            assert dbg(h, name, buf, 64, write) == -1     # a handle of 0 envs: every plane holds 0 bytes
            assert b'holds 0 bytes, the buffer 64' in L.bioim_last_error()
    for n in (0, -3, 4):        # none, negative, more than the handle's envs
        assert L.bioim_copy_state_rows(h, idp, n, buf) == -1
        assert b'bioim_copy_state_rows: n must lie in' in L.bioim_last_error()
        assert L.bioim_load_state(h, idp, n, buf) == -1
        assert b'bioim_load_state: n must lie in' in L.bioim_last_error()
        assert L.bioim_clone_envs(h, idp, idp, n) == -1
        assert b'bioim_clone_envs: n must lie in' in L.bioim_last_error()
