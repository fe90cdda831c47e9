"""bioim_induced_accel (include/bioim.h): the header declares it, the binding
lists it, and its argument checks return BIOIM_E_ARG (-1) with a message before
any device call, in the header's order; the ValueError paths of
InducedAccelerations.eval's argument check, the contributor names and write_sto
need no device either.  All of this runs without a GPU (the pattern of
test_joint_reaction_abi.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'bioim_induced_accel'


def _lib_or_skip():
    from bioimitation import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libbioim.so not built')
    return _lib, _lib.load()


def test_header_declares_the_call():
    txt = open(os.path.join(REPO, 'include', 'bioim.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    code = ' '.join(code.split())
    assert ('int bioim_induced_accel(bioim_handle_t *h, int n, const void *q, const void *u , const void *ft , '
            'const void *tau_act , const void *ext , int kind, const uint8_t *cactive , const void *cpoint , '
            'double force_threshold, void *accel , void *com_accel , void *reaction , void *cpoint_out , '
            'uint8_t *cactive_out , int32_t *status );') in code
    assert 'enum { BIOIM_IA_FORCE = 0, BIOIM_IA_POINT = 1 };' in code
    assert code.index('int bioim_joint_reaction(') < code.index('int bioim_induced_accel(') < code.index('int bioim_osim(')
    doc = txt[txt.index('Induced accelerations ('):txt.index('enum { BIOIM_IA_FORCE')]
    doc = ' '.join(doc.replace('\n *', ' ').split())
    for word in ("OpenSim's InducedAccelerations", 'neither read nor written', 'fp64 handles only',
                 'Schur complement J M^-1 J^T on a floating base', 'NC = 6 + ncforce + nmuscle', 'in this fixed order',
                 'g(q) (BIOIM_ID_GRAVITY)', '-c(q, u) (BIOIM_ID_CORIOLIS, negated)', 'which is what bioim_id_eval applies',
                 'exactly 0 for a constrained foot', 'the coordinate limit forces', 'tau_act [n][ndof]',
                 "bioim_joint_reaction's convention", "a moving point's own-coordinate term",
                 "sum to bioim_muscle_eval's tau", 'the sum of all Q_c', 'A_c = M^-1 Q_c',
                 "forward-dynamics acceleration", 'M A_c - sum_f J_f^T lambda_{c,f} = Q_c',
                 'J_f A_c + [c is velocity or total] beta_f = 0', '(Omega_d x P_f + V_d)',
                 "the composite body that carries force f's spheres", "q(t) = q + u t", "at q'' = 0",
                 '3 on spatial topologies, 2 (x, y) on planar ones', 'planar reaction z is exactly 0',
                 'not forward dynamics', 'or neither', 'exceeds force_threshold',
                 'sum_s fn_s P_s / sum_s fn_s', 'ignored in FORCE mode', 'any may be NULL, not all',
                 'd^2/dt^2 com(q + u t)', 'Zeros in FORCE mode and for unconstrained feet', 'what was used',
                 '-2 for a pivot <= 0 or a NaN', 'The outputs are then zeros', 'u NULL: zeros', 'bit for bit',
                 'BIOIM_E_ARG', 'in this order', 'ft on a model without muscles', 'kind outside 0..1',
                 'exactly one of cactive / cpoint', 'force_threshold not finite or < 0', 'every output NULL',
                 'an fp32 handle', 'n == 0 returns BIOIM_OK', 'synchronizes nothing'):
        assert word in doc, word


def test_binding_lists_it():
    from bioimitation import _lib
    assert NAME in _lib.EXPORTS
    from bioimitation import induced_accelerations as ia
    assert ia.KEYS == ('accel', 'com_accel', 'reaction', 'cpoint', 'cactive', 'status')
    assert ia.DEFAULT_WANT == ('accel',)
    assert ia.KINDS == {'force': 0, 'point': 1}


def test_library_exports_it():
    _lib, L = _lib_or_skip()
    assert hasattr(L, NAME)
    at = L.bioim_induced_accel.argtypes
    assert at is not None and len(at) == 17
    assert at[1] is C.c_int and at[7] is C.c_int and at[10] is C.c_double


def test_refusals_come_before_any_device_call_in_order():
    """Each refusal of the header, in its order.  The handle is a zeroed block
    at least as large as the library's handle: its muscle count is 0 (a torque
    model) and its precision is not 64, so the last check (an fp32 handle) ends
    every call that passes the others, and none reaches a launch.  Each call
    fails the check it is about, passes all before it and fails every later one
    it can."""
    _lib, L = _lib_or_skip()
    from bioimitation import packdef
    blk = C.create_string_buffer(C.sizeof(packdef.ModelPack) + 65536)
    h = C.cast(blk, C.c_void_p)
    p = C.cast(C.create_string_buffer(64), C.c_void_p)
    nan, inf = float('nan'), float('inf')

    def refused(msg, *args):
        assert L.bioim_induced_accel(*args) == -1, msg
        err = L.bioim_last_error()
        assert err.startswith(b'bioim_induced_accel:') and msg in err, (msg, err)
    N = None
    #                               h  n   q  u  ft tau ext kind ca cp thr   accel com reac cpo cao status
    refused(b'null handle',         N, 1,  p, p, N, p,  p,  1,   p, p, 0.0,  p, p, p, p, p, p)
    refused(b'null handle',         N, -1, N, N, p, N,  N,  2,   p, N, nan,  N, N, N, N, N, N)
    refused(b'negative n',          h, -1, N, N, p, N,  N,  2,   p, N, nan,  N, N, N, N, N, N)
    refused(b'null q',              h, 1,  N, N, p, N,  N,  2,   p, N, nan,  N, N, N, N, N, N)
    refused(b'ft on a model without muscles', h, 1, p, N, p, N, N, 2, p, N, nan, N, N, N, N, N, N)
    refused(b'ft on a model without muscles', h, 0, N, N, p, N, N, 2, p, N, nan, N, N, N, N, N, N)
    for kind in (-1, 2, 1 << 20):
        refused(b'kind must be',    h, 1,  p, N, N, N,  N,  kind, p, N, nan, N, N, N, N, N, N)
    for ca, cp in ((p, N), (N, p)):
        refused(b'cactive and cpoint go together', h, 1, p, N, N, N, N, 1, ca, cp, nan, N, N, N, N, N, N)
        refused(b'cactive and cpoint go together', h, 1, p, N, N, N, N, 0, ca, cp, -1.0, N, N, N, N, N, N)
    for thr in (nan, inf, -inf, -1e-300):
        refused(b'force_threshold must be', h, 1, p, N, N, N, N, 1, p, p, thr, N, N, N, N, N, N)
        refused(b'force_threshold must be', h, 1, p, N, N, N, N, 0, N, N, thr, N, N, N, N, N, N)
    for kind in (0, 1):
        refused(b'no output requested', h, 1, p, p, N, p, p, kind, N, N, 0.0, N, N, N, N, N, N)
        refused(b'no output requested', h, 0, N, N, N, N, N, kind, p, p, 5.0, N, N, N, N, N, N)
    for k in range(6):
        outs = [N] * 6
        outs[k] = p
        refused(b'fp64 handles only', h, 1, p, p, N, p, p, 1, p, p, 0.0, *outs)
        refused(b'fp64 handles only', h, 0, N, N, N, N, N, 0, N, N, 0.0, *outs)
    src = open(os.path.join(REPO, 'bioimitation-gym_amd', 'csrc', 'bioim_step.hip')).read()
    body = src[src.index('int bioim_induced_accel(bioim_handle_t *h'):]
    body = body[:body.index('\n}\n')]
    order = [body.index(m) for m in ('null handle', 'negative n', 'null q"', 'ft on a model without muscles',
                                     'kind must be', 'cactive and cpoint go together', 'force_threshold must be',
                                     'no output requested', 'fp64 handles only', 'if (n == 0) return 0',
                                     'hipSetDevice')]
    assert order == sorted(order)


def test_eval_argument_errors_need_no_device():
    from bioimitation.induced_accelerations import DEFAULT_WANT, KEYS, check_args
    nd, nm, nb, nf, n = 9, 14, 7, 2, 3
    q, ft, ext = np.zeros((n, nd)), np.zeros((n, nm)), np.zeros((n, nb, 6))
    ca, cp = np.zeros((n, nf), dtype=np.uint8), np.zeros((n, nf, 3))
    assert check_args(nd, nm, nb, nf, q) == (n, DEFAULT_WANT)
    assert check_args(nd, nm, nb, nf, q, q, ft, q, ext, 'force', ca, cp, 2.5, KEYS) == (n, KEYS)
    assert check_args(nd, nm, nb, nf, q, cactive=ca.astype(bool), cpoint=cp, want='status') == (n, ('status',))
    assert check_args(nd, nm, nb, nf, np.zeros((0, nd)), want=KEYS) == (0, KEYS)
    assert check_args(nd, 0, nb, nf, q.astype(np.float32), ext=ext.astype(np.int64)) == (n, DEFAULT_WANT)
    for kw, msg in ((dict(want=()), 'nothing requested'),
                    (dict(want=('accel', 'force')), "unknown key 'force'"),
                    (dict(kind='weld'), "unknown kind 'weld'"),
                    (dict(cactive=ca), 'cactive and cpoint go together'),
                    (dict(cpoint=cp), 'cactive and cpoint go together'),
                    (dict(force_threshold=-1.0), 'force_threshold must be finite and >= 0'),
                    (dict(force_threshold=float('nan')), 'force_threshold must be finite and >= 0'),
                    (dict(force_threshold='x'), 'force_threshold must be a number'),
                    (dict(u=np.zeros((n, nd + 1))), 'u must have shape (n, 9)'),
                    (dict(tau_act=np.zeros((n + 1, nd))), 'tau_act has 4 rows, q has 3'),
                    (dict(ft=np.zeros((n, nm - 1))), 'ft must have shape (n, 14)'),
                    (dict(ext=np.zeros((n, nb, 3))), 'ext must have shape (n, 7, 6)'),
                    (dict(cactive=np.zeros((n, 3)), cpoint=cp), 'cactive must have shape (n, 2)'),
                    (dict(cactive=ca, cpoint=np.zeros((n, nf))), 'cpoint must have shape (n, 2, 3)'),
                    (dict(u=np.zeros((n, nd), dtype=complex)), 'u must hold real numbers'),
                    (dict(ft=np.zeros((n, nm), dtype=bool)), 'ft must hold real numbers')):
        with pytest.raises(ValueError, match=re.escape(msg)):
            check_args(nd, nm, nb, nf, q, **kw)
    with pytest.raises(ValueError, match='q is required'):
        check_args(nd, nm, nb, nf, None)
    with pytest.raises(ValueError, match=re.escape('q must have shape (n, 9)')):
        check_args(nd, nm, nb, nf, np.zeros(nd))
    with pytest.raises(ValueError, match='the model has no muscles'):
        check_args(nd, 0, nb, nf, q, ft=np.zeros((n, 0)))


def _names(env_id):
    from bioimitation.induced_accelerations import contributor_names, dof_names
    from bioimitation.obslayout import load_names
    from bioimitation.registry import load_pack
    pk, names = load_pack(env_id), load_names(env_id)
    return pk, names, contributor_names(pk, names), dof_names(pk, names)


def test_contributor_names():
    pk, names, cols, dofs = _names('MuscleWalkingImitation2D-v0')
    assert len(cols) == 6 + pk.ncforce + pk.nmuscle == 22 and len(set(cols)) == len(cols)
    assert cols[:2] == ['gravity', 'velocity'] and cols[2:4] == list(names['cforces'])
    assert cols[4:7] == ['limits', 'actuators', 'external'] and cols[-1] == 'total'
    assert cols[7:-1] == list(names['muscles']) and 'soleus_r' in cols
    assert len(dofs) == pk.ndof and 'pelvis_ty' in dofs
    pk, names, cols, dofs = _names('TorqueLockedKneeImitation2D-v0')
    assert len(cols) == 6 + pk.ncforce == 8 and cols[-4:] == ['limits', 'actuators', 'external', 'total']
    from bioimitation.induced_accelerations import contributor_names
    assert contributor_names(pk, {})[2:4] == ['contact_0', 'contact_1']      # a pack without force names


def test_write_sto_columns_and_round_trip(tmp_path):
    from bioimitation import induced_accelerations as ia
    from bioimitation import storage
    pk, names, cols, dofs = _names('MuscleWalkingImitation2D-v0')
    n, nc = 5, len(cols)
    rng = np.random.default_rng(3)
    out = dict(accel=rng.normal(size=(n, nc, pk.ndof)), com_accel=rng.normal(size=(n, nc, 3)))
    t = np.arange(n) * 0.01
    path = str(tmp_path / 'ia_pelvis_ty.sto')
    ia.write_sto(path, t, out, 'pelvis_ty', contributors=cols, coords=dofs)
    _, labels, data = storage.read_sto(path)
    assert list(labels) == ['time'] + cols
    assert np.allclose(data[:, 0], t) and np.allclose(data[:, 1:], out['accel'][:, :, dofs.index('pelvis_ty')])
    path = str(tmp_path / 'ia_com.sto')
    ia.write_sto(path, t, out, 'com', contributors=cols)
    _, labels, data = storage.read_sto(path)
    assert list(labels) == ['time'] + [f'{c}_{x}' for c in cols for x in 'xyz']
    assert np.allclose(data[:, 1:], out['com_accel'].reshape(n, -1))
    for args, msg in ((('knee',), 'unknown coordinate'), ((99,), 'dof index 99')):
        with pytest.raises(ValueError, match=msg):
            ia.write_sto(path, t, out, *args, contributors=cols, coords=dofs)
    with pytest.raises(ValueError, match="needs 'com_accel'"):
        ia.write_sto(path, t, dict(accel=out['accel']), 'com', contributors=cols)
    with pytest.raises(ValueError, match='contributor names'):
        ia.write_sto(path, t, out, 'com')
