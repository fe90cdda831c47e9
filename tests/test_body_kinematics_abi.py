"""bioim_body_kin (include/bioim.h): the header declares it, the binding lists
it, and its argument checks return BIOIM_E_ARG (-1) with a message before any
device call, in the header's order; the ValueError paths of
BodyKinematics.eval's argument check, the storage labels and the hazard gate's
kernel list need no device either.  All of this runs without a GPU (the
pattern of test_induced_accel_abi.py)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'bioim_body_kin'
R3D = 'MuscleRunningImitation3D-v0'


def _lib_or_skip():
    from bioimitation import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libbioim.so not built')
    return _lib, _lib.load()


def test_header_declares_the_call():
    txt = open(os.path.join(REPO, 'include', 'bioim.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    code = ' '.join(code.split())
    assert ('int bioim_body_kin(bioim_handle_t *h, int n, const void *q, const void *u , const void *qdd , int npt, '
            'const int32_t *pt_body , const void *pt_local , int flags , void *origin , void *com , void *orient , '
            'void *rot , void *system , void *momentum , void *energy , void *point );') in code
    assert '#define BIOIM_BK_MAX_POINTS 64' in code and '#define BIOIM_BK_LOCAL 1' in code
    assert code.index('int bioim_induced_accel(') < code.index('int bioim_body_kin(') < code.index('int bioim_osim(')
    doc = txt[txt.index('Body kinematics ('):txt.index('#define BIOIM_BK_MAX_POINTS')]
    doc = ' '.join(doc.replace('\n *', ' ').split())
    for word in ("OpenSim's BodyKinematics and PointKinematics", 'neither read nor written', 'Both precisions',
                 'u, qdd NULL: zeros, bit for bit', "sum over the dofs d on k's root path of S_d q''_d",
                 'HOST array', '-1 = ground', 'before any launch', 'BIOIM_BK_MAX_POINTS is 64',
                 'any may be NULL, not all', '[n][nosbody][3][3]', 'osbody.com', 'body-fixed XYZ angles of R = Rx Ry Rz',
                 '[n][nosbody][9]', 'about the whole-body mass centre', '-m g . C', 'a ground point is fixed',
                 "express_results_in_body_local_frame", 'stay in the ground frame', 'No status output',
                 'does not depend on n', 'bit for bit', 'BIOIM_E_ARG', 'in this order', 'npt < 0 or npt > BIOIM_BK_MAX_POINTS',
                 'a null point table with npt > 0', 'outside [-1, nosbody)', 'unknown flag bits', 'null q with n > 0',
                 'every output NULL', 'n == 0 returns BIOIM_OK', 'synchronizes nothing'):
        assert word in doc, word


def test_binding_lists_it():
    from bioimitation import _lib
    from bioimitation import body_kinematics as bk
    assert NAME in _lib.EXPORTS
    assert bk.KEYS == ('origin', 'com', 'orient', 'rot', 'system', 'momentum', 'energy', 'point')
    assert bk.DEFAULT_WANT == ('com', 'system')
    assert (bk.LOCAL, bk.MAX_POINTS) == (1, 64)


def test_library_exports_it():
    _lib, L = _lib_or_skip()
    assert hasattr(L, NAME)
    at = L.bioim_body_kin.argtypes
    assert at is not None and len(at) == 17
    assert at[1] is C.c_int and at[5] is C.c_int and at[8] is C.c_int
    assert at[6] is C.POINTER(C.c_int32) and at[7] is C.POINTER(C.c_double)
    assert all(a is C.c_void_p for a in at[:1] + at[2:5] + at[9:])


def test_refusals_come_before_any_device_call_in_order():
    """Each refusal of the header, in its order.  The handle is a zeroed block
    at least as large as the library's handle: its model has no OpenSim bodies,
    so only ground points pass the body check, and every call ends at the last
    check at the latest (no output requested): none reaches a launch."""
    _lib, L = _lib_or_skip()
    from bioimitation import packdef
    blk = C.create_string_buffer(C.sizeof(packdef.ModelPack) + 65536)
    h = C.cast(blk, C.c_void_p)
    p = C.cast(C.create_string_buffer(64), C.c_void_p)
    ground, bad_lo, bad_hi = (C.c_int32 * 2)(-1, -1), (C.c_int32 * 2)(-1, -2), (C.c_int32 * 2)(-1, 0)
    loc = (C.c_double * 6)()
    N = None

    def refused(msg, *args):
        assert L.bioim_body_kin(*args) == -1, msg
        err = L.bioim_last_error()
        assert err.startswith(b'bioim_body_kin:') and msg in err, (msg, err)
    #                              h  n   q  u  qdd npt pt_body pt_local flags  8 outputs
    refused(b'null handle',        N, 1,  p, p, p,  0,  N,      N,       0,     p, p, p, p, p, p, p, p)
    refused(b'null handle',        N, -1, N, N, N,  -1, N,      N,       2,     N, N, N, N, N, N, N, N)
    refused(b'negative n',         h, -1, N, N, N,  -1, N,      N,       2,     N, N, N, N, N, N, N, N)
    for npt in (-1, 65, 1 << 20):
        refused(b'npt must be in', h, 1,  N, N, N,  npt, N,     N,       2,     N, N, N, N, N, N, N, N)
    for pb, pl in ((N, loc), (ground, N), (N, N)):
        refused(b'null point table', h, 1, N, N, N, 2,  pb,     pl,      2,     N, N, N, N, N, N, N, N)
    for pb in (bad_lo, bad_hi):
        refused(b'outside [-1, nosbody)', h, 1, N, N, N, 2, pb, loc,     2,     N, N, N, N, N, N, N, N)
    for flags in (2, 3, -1, 1 << 20):
        refused(b'unknown flag bits', h, 1, N, N, N, 2, ground, loc,     flags, N, N, N, N, N, N, N, N)
    for flags in (0, 1):
        refused(b'null q',         h, 1,  N, p, p,  2,  ground, loc,     flags, N, N, N, N, N, N, N, N)
        refused(b'no output requested', h, 1, p, N, N, 2, ground, loc,   flags, N, N, N, N, N, N, N, N)
        refused(b'no output requested', h, 0, N, N, N, 0, N,    N,       flags, N, N, N, N, N, N, N, N)


def _names():
    from bioimitation.obslayout import load_names
    from bioimitation.registry import load_pack
    return load_pack(R3D), list(load_names(R3D)['bodies'])


def test_check_args_refusals():
    from bioimitation import body_kinematics as bk
    pk, bodies = _names()
    nd = pk.ndof
    q = np.zeros((5, nd))
    toe = [('calcn_r', (0.18, 0.0, 0.0)), ('ground', (0, 0, 0))]
    n, want, pb, pl = bk.check_args(nd, bodies, q, q, q, toe, False, ('com', 'point'))
    assert (n, want) == (5, ('com', 'point')) and pb.dtype == np.int32 and pl.dtype == np.float64
    assert pb.tolist() == [bodies.index('calcn_r'), -1] and pl.tolist() == [[0.18, 0, 0], [0, 0, 0]]
    assert bk.check_args(nd, bodies, q.astype(np.float32), want='rot')[1] == ('rot',)
    assert bk.check_args(nd, bodies, np.zeros((0, nd)))[:2] == (0, bk.DEFAULT_WANT)
    assert bk.check_args(nd, bodies, q)[2].shape == (0,)

    def refused(msg, *a, **kw):
        with pytest.raises(ValueError, match=msg) as e:
            bk.check_args(nd, bodies, *a, **kw)
        assert str(e.value).startswith('body kinematics: ')
    refused('q is required', None)
    refused(r'q must have shape \(n, %d\)' % nd, np.zeros((5, nd + 1)))
    refused(r'q must have shape \(n, %d\)' % nd, np.zeros(nd))
    refused(r'u must have shape', q, np.zeros((5, nd, 1)))
    refused('u has 4 rows, q has 5', q, np.zeros((4, nd)))
    refused('qdd has 6 rows, q has 5', q, q, np.zeros((6, nd)))
    refused('q must hold real numbers', q.astype(bool))
    refused('qdd must hold real numbers', q, None, q.astype(complex))
    refused('u must hold real numbers', q, [['a'] * nd] * 5)
    refused('nothing requested', q, want=())
    refused("unknown key 'velocity'", q, want=('com', 'velocity'))
    refused(r"unknown body 'toe_r'; choose from \[.*'calcn_r'.*\] or 'ground'", q, points=[('toe_r', (0, 0, 0))])
    refused(r'points\[1\] must be \(body name, \(x, y, z\)\)', q, points=[toe[0], 'calcn_r'])
    refused(r"points\[0\]'s location must have shape \(3,\)", q, points=[('calcn_r', (0, 0))])
    refused(r"points\[0\]'s location must hold real numbers", q, points=[('calcn_r', (0, 0, 1j))])
    refused('65 points; one call takes at most 64', q, points=[toe[0]] * 65)
    assert bk.check_args(nd, bodies, q, points=[toe[0]] * 64)[2].shape == (64,)
    assert np.issubdtype(np.asarray(q.astype(int)).dtype, np.integer) and bk.check_args(nd, bodies, q.astype(int))[0] == 5


def test_write_sto_labels_are_the_committed_tables(tmp_path):
    """write_sto's labels are those of the committed reference table that
    refmotion.synthesize_reference wrote and load_reference_tables reads."""
    from bioimitation import body_kinematics as bk, storage
    import bioimitation
    pk, bodies = _names()
    n, nb = 3, len(bodies)
    rng = np.random.default_rng(0)
    out = dict(com=rng.normal(size=(n, nb, 3, 3)), orient=rng.normal(size=(n, nb, 3, 3)), system=rng.normal(size=(n, 3, 3)))
    files = bk.write_sto(str(tmp_path / 'out'), [0.0, 0.01, 0.02], out, bodies=bodies)
    assert [os.path.basename(f) for f in files] == [f'task_BodyKinematics_{k}_global.sto' for k in ('pos', 'vel', 'acc')]
    committed = os.path.join(os.path.dirname(bioimitation.__file__), 'data', '3D', 'walking_reference_data',
                             'task_BodyKinematics_pos_global.sto')
    want = storage.read_sto(committed)[1]
    for j, f in enumerate(files):
        _, labels, data = storage.read_sto(f)
        assert labels == want
        assert np.abs(data[:, 1:4] - out['com'][:, 0, j]).max() < 1e-9 and np.abs(data[:, 4:7] - out['orient'][:, 0, j]).max() < 1e-9
        assert np.abs(data[:, -3:] - out['system'][:, j]).max() < 1e-9
    res = bk.Result(out)
    res.bodies, res.local = bodies, True
    assert os.path.basename(bk.write_sto(str(tmp_path / 'loc'), [0, 1, 2], res)[1]) == 'task_BodyKinematics_vel_bodyLocal.sto'
    with pytest.raises(ValueError, match="body kinematics: write_sto needs 'orient'"):
        bk.write_sto(str(tmp_path / 'x'), [0, 1, 2], dict(com=out['com'], system=out['system']), bodies=bodies)
    with pytest.raises(ValueError, match='body kinematics: write_sto needs the body names'):
        bk.write_sto(str(tmp_path / 'x'), [0, 1, 2], out)
    with pytest.raises(ValueError, match='for 2 times and 13 bodies'):
        bk.write_sto(str(tmp_path / 'x'), [0, 1], out, bodies=bodies)


def test_hazard_gate_scans_the_kernel():
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import hazard_gate
    assert 'bk_kernel' in hazard_gate.KERNELS
