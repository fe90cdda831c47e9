"""bioim_joint_reaction (include/bioim.h): the header declares it, the binding
lists it, and its argument checks return BIOIM_E_ARG (-1) with a message before
any device call, in the header's order; the ValueError paths of
JointReaction.eval's argument check, the joint naming and write_sto need no
device either.  All of this runs without a GPU (the pattern of
test_ik_abi.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'bioim_joint_reaction'


def _lib_or_skip():
    from bioimitation import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libbioim.so not built')
    return _lib, _lib.load()


def test_header_declares_the_call():
    txt = open(os.path.join(REPO, 'include', 'bioim.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    code = ' '.join(code.split())
    assert ('int bioim_joint_reaction(bioim_handle_t *h, int n, const void *q, const void *u , const void *qdd , '
            'const void *ft , const void *ext , int flags, int frame, void *reaction , void *point , '
            'void *tau_joint , void *muscle_wrench );') in code
    assert 'enum { BIOIM_JR_GROUND = 0, BIOIM_JR_CHILD = 1, BIOIM_JR_PARENT = 2 };' in code
    assert '#define BIOIM_JR_CONTACT 1' in code
    doc = txt[txt.index('Joint reaction analysis ('):txt.index('enum { BIOIM_JR_GROUND')]
    doc = ' '.join(doc.replace('\n *', ' ').split())
    for word in ("OpenSim's JointReaction", 'neither read nor written',
                 'W_k = I_k a_k + v_k x* I_k v_k - (gravity on k)', 'if flag CONTACT', 'ext_k',
                 "a_k = AL_k + sum over the dofs d on k's root path of S_d q''_d",
                 'F_b = sum over k in subtree(b) of W_k', 'c_b = o_b - R_b R_mb^T p_mb',
                 'o_b in every shipped pack', "muscle_path's activity rule", 'q < lo || q > hi',
                 'moving points sit at their function values', 'Ft_m (e_{j->j+1} - e_{j-1->j})',
                 "-Ft g in muscle_path's notation", 'mobility force, not a body force', 'It is not part of F',
                 'Coordinate limit forces, coordinate actuators and reserves', 'tau_joint_d = S_d . F_{cb(d)}',
                 'both about the same point', 'rotates `reaction` only', 'ground for the root',
                 'keep all six components', 'have no row', 'bit for bit', 'BIOIM_E_ARG', 'in this order',
                 'ft on a model without muscles', 'unknown flag bits', 'frame outside 0..2', 'every output NULL',
                 'n == 0 returns BIOIM_OK', 'synchronizes nothing'):
        assert word in doc, word


def test_binding_lists_it():
    from bioimitation import _lib
    assert NAME in _lib.EXPORTS
    from bioimitation import joint_reaction as jr
    assert jr.KEYS == ('reaction', 'point', 'tau_joint', 'muscle_wrench')
    assert jr.DEFAULT_WANT == ('reaction',)
    assert jr.FRAMES == {'ground': 0, 'child': 1, 'parent': 2} and jr.CONTACT == 1


def test_library_exports_it():
    _lib, L = _lib_or_skip()
    assert hasattr(L, NAME)
    at = L.bioim_joint_reaction.argtypes
    assert at is not None and len(at) == 13
    assert at[1] is C.c_int and at[7] is C.c_int and at[8] is C.c_int


def test_refusals_come_before_any_device_call_in_order():
    """Each refusal of the header, in its order.  The handle is a zeroed block
    at least as large as the library's handle (the trick of
    test_muscle_analysis_abi.py): its muscle count is 0, so it stands for a
    torque model.  Each call below fails the check it is about and passes all
    before it, while failing every later one it can; none may reach a launch,
    so the last check (every output NULL) ends those that pass the others."""
    _lib, L = _lib_or_skip()
    from bioimitation import packdef
    blk = C.create_string_buffer(C.sizeof(packdef.ModelPack) + 65536)
    h = C.cast(blk, C.c_void_p)
    p = C.cast(C.create_string_buffer(64), C.c_void_p)

    def refused(msg, *args):
        assert L.bioim_joint_reaction(*args) == -1, msg
        err = L.bioim_last_error()
        assert err.startswith(b'bioim_joint_reaction:') and msg in err, (msg, err)
    #                          h    n   q     u     qdd   ft    ext  flags frame reac  point tau   mw
    refused(b'null handle', None, 1, p, p, p, None, p, 1, 1, p, p, p, p)
    refused(b'null handle', None, -1, None, None, None, p, None, 2, 3, None, None, None, None)
    refused(b'negative n', h, -1, None, None, None, p, None, 2, 3, None, None, None, None)
    refused(b'null q', h, 1, None, None, None, p, None, 2, 3, None, None, None, None)
    refused(b'ft on a model without muscles', h, 1, p, None, None, p, None, 2, 3, None, None, None, None)
    refused(b'ft on a model without muscles', h, 0, None, None, None, p, None, 2, 3, None, None, None, None)
    for flags in (2, 3, 1 << 8, -2):
        refused(b'unknown flag bits', h, 1, p, None, None, None, None, flags, 3, None, None, None, None)
    for frame in (-1, 3, 1 << 20):
        refused(b'frame must be', h, 1, p, p, p, None, p, 1, frame, None, None, None, None)
    for flags in (0, 1):
        for frame in (0, 1, 2):
            refused(b'no output requested', h, 1, p, p, p, None, p, flags, frame, None, None, None, None)
    # n == 0: no q needed, the later checks still come, and with an output the call is OK without a launch
    refused(b'unknown flag bits', h, 0, None, None, None, None, None, 4, 0, p, None, None, None)
    refused(b'no output requested', h, 0, None, None, None, None, None, 0, 0, None, None, None, None)
    for outs in ((p, None, None, None), (None, p, None, None), (None, None, p, None), (None, None, None, p)):
        assert L.bioim_joint_reaction(h, 0, None, None, None, None, None, 1, 2, *outs) == 0
    src = open(os.path.join(REPO, 'bioimitation-gym_amd', 'csrc', 'bioim_step.hip')).read()
    body = src[src.index('int bioim_joint_reaction(bioim_handle_t *h'):]
    body = body[:body.index('\n}\n')]
    order = [body.index(m) for m in ('null handle', 'negative n', 'null q"', 'ft on a model without muscles',
                                     'unknown flag bits', 'frame must be', 'no output requested',
                                     'if (n == 0) return 0', 'hipSetDevice')]
    assert order == sorted(order)


def test_eval_argument_errors_need_no_device():
    from bioimitation.joint_reaction import DEFAULT_WANT, KEYS, check_args
    nd, nm, nb, n = 9, 14, 7, 3
    q, ft, ext = np.zeros((n, nd)), np.zeros((n, nm)), np.zeros((n, nb, 6))
    assert check_args(nd, nm, nb, q) == (n, DEFAULT_WANT)
    assert check_args(nd, nm, nb, q, q, q, ft, ext, 'ground', 'parent', KEYS) == (n, KEYS)
    assert check_args(nd, nm, nb, q, want='point') == (n, ('point',))
    assert check_args(nd, nm, nb, np.zeros((0, nd)), want=KEYS) == (0, KEYS)
    assert check_args(nd, 0, nb, q.astype(np.float32), ext=ext.astype(np.int64)) == (n, DEFAULT_WANT)
    for kw, msg in ((dict(want=()), 'nothing requested'),
                    (dict(want=('reaction', 'force')), "unknown key 'force'"),
                    (dict(frame='body'), "unknown frame 'body'"),
                    (dict(on='ground'), "unknown on='ground'"),
                    (dict(u=np.zeros((n, nd + 1))), 'u must have shape (n, 9)'),
                    (dict(qdd=np.zeros((n + 1, nd))), 'qdd has 4 rows, q has 3'),
                    (dict(ft=np.zeros((n, nm - 1))), 'ft must have shape (n, 14)'),
                    (dict(ext=np.zeros((n, nb * 6))), 'ext must have shape (n, 7, 6)'),
                    (dict(ext=np.zeros((n, nb, 3))), 'ext must have shape (n, 7, 6)'),
                    (dict(u=np.zeros((n, nd), dtype=complex)), 'u must hold real numbers'),
                    (dict(ft=np.zeros((n, nm), dtype=bool)), 'ft must hold real numbers')):
        with pytest.raises(ValueError, match=re.escape(msg)):
            check_args(nd, nm, nb, q, **kw)
    with pytest.raises(ValueError, match='q is required'):
        check_args(nd, nm, nb, None)
    with pytest.raises(ValueError, match=re.escape('q must have shape (n, 9)')):
        check_args(nd, nm, nb, np.zeros(nd))
    with pytest.raises(ValueError, match='the model has no muscles'):
        check_args(nd, 0, nb, q, ft=np.zeros((n, 0)))


def test_joint_names_walking2d():
    from bioimitation.joint_reaction import JointTable
    t = JointTable('MuscleWalkingImitation2D-v0')
    assert t.joints == ['ground_pelvis', 'hip_r', 'knee_r', 'ankle_r', 'hip_l', 'knee_l', 'ankle_l']
    assert t.child_bodies == ['pelvis', 'femur_r', 'tibia_r', 'talus_r', 'femur_l', 'tibia_l', 'talus_l']
    assert t.parent_bodies == ['ground', 'pelvis', 'femur_r', 'tibia_r', 'pelvis', 'femur_l', 'tibia_l']
    assert t.index('knee_l') == 5 and t.index('ground_pelvis') == 0
    # the welded joints (back: torso; subtalar, mtp: calcn and toes) lie inside composite bodies
    assert {"torso's inboard joint", "calcn_r's inboard joint", "toes_l's inboard joint"} <= set(t.inner)
    # a welded joint has no coordinates, so the pack does not carry its name: the reason says so and lists them
    assert not {'back', 'subtalar_r', 'mtp_l'} & set(t.inner)
    for name in ('back', 'subtalar_r', 'mtp_l'):
        with pytest.raises(KeyError) as ei:
            t.index(name)
        msg = ei.value.args[0]
        assert 'welded joint, which has no coordinates' in msg and "calcn_r's inboard joint" in msg
        assert 'are locked' not in msg
    assert t.inner["torso's inboard joint"] == "welded or locked inside composite body 'pelvis'"


def test_joint_names_locked_knee3d():
    from bioimitation.joint_reaction import JointTable
    t = JointTable('MuscleLockedKneeImitation3D-v0')
    assert t.joints == ['ground_pelvis', 'hip_r', 'knee_r', 'ankle_r', 'hip_l'] and len(t.joints) == 5
    assert 'knee_l' not in t.joints
    assert t.child_bodies[4] == 'femur_l' and t.parent_bodies[4] == 'pelvis'
    for name, coord in (('knee_l', 'knee_angle_l'), ('ankle_l', 'ankle_angle_l'), ('back', 'lumbar_extension')):
        assert t.inner[name] == f'its coordinates ({coord}) are locked, so the pack merges its child into the parent body'
        with pytest.raises(KeyError) as ei:
            t.index(name)
        assert t.inner[name] in ei.value.args[0] and 'welded joint, which has no coordinates' not in ei.value.args[0]
    with pytest.raises(KeyError, match='welded joint, which has no coordinates'):
        t.index('subtalar_l')
    assert "tibia_l's inboard joint" in t.inner and 'femur_l' in t.inner["tibia_l's inboard joint"]


def test_write_sto_columns_and_round_trip(tmp_path):
    from bioimitation import joint_reaction as jr
    from bioimitation import storage
    t = jr.JointTable('MuscleLockedKneeImitation3D-v0')
    rng = np.random.default_rng(5)
    n = 4
    out = jr.Result(reaction=rng.normal(size=(n, 5, 6)) * 100, point=rng.normal(size=(n, 5, 3)))
    out.table, out.frame, out.on = t, 'child', 'child'
    time = 0.01 * np.arange(n)
    path = str(tmp_path / 'jr.sto')
    jr.write_sto(path, time, out)
    header, labels, data = storage.read_sto(path)
    assert labels[0] == 'time' and len(labels) == 1 + 9 * 5
    assert labels[1:10] == [f'ground_pelvis_on_pelvis_in_pelvis_{c}' for c in
                            ('fx', 'fy', 'fz', 'mx', 'my', 'mz', 'px', 'py', 'pz')]
    assert labels[19] == 'knee_r_on_tibia_r_in_tibia_r_fx' and labels[-1] == 'hip_l_on_femur_l_in_femur_l_pz'
    assert data.shape == (n, 46)
    np.testing.assert_allclose(data[:, 0], time, atol=1e-10)
    want = np.concatenate([out['reaction'], out['point']], axis=2).reshape(n, -1)
    np.testing.assert_allclose(data[:, 1:], want, atol=0.6e-10)   # the file keeps 10 decimals
    # the other labellings
    assert t.columns('ground', 'parent')[9] == 'hip_r_on_pelvis_in_ground_fx'
    assert t.columns('parent', 'child')[18] == 'knee_r_on_tibia_r_in_femur_r_fx'
    assert t.columns('parent', 'child')[0] == 'ground_pelvis_on_pelvis_in_ground_fx'
    assert t.columns('child', 'parent')[0] == 'ground_pelvis_on_ground_in_pelvis_fx'
    jr.write_sto(path, time, dict(out), table=t, frame='ground', on='parent')
    assert storage.read_sto(path)[1][10] == 'hip_r_on_pelvis_in_ground_fx'
    with pytest.raises(ValueError, match="needs 'point'"):
        jr.write_sto(path, time, dict(reaction=out['reaction']), table=t)
    with pytest.raises(ValueError, match='needs the joint table'):
        jr.write_sto(path, time, dict(out))
    with pytest.raises(ValueError, match='for 3 times'):
        jr.write_sto(path, time[:3], out)


def test_realize_report_entry():
    """bioim_realize_report, the REALIZE that VectorEnv.joint_reaction uses: declared, bound, and refused in the
    header's order before any device call (the zeroed handle has never had an RK budget, so a call that passes
    the checks may only be made with n = 0)."""
    txt = open(os.path.join(REPO, 'include', 'bioim.h')).read()
    code = ' '.join(re.sub(r'/\*.*?\*/', '', txt, flags=re.S).split())
    assert 'int bioim_realize_report(bioim_handle_t *h, const int32_t *env_ids, int n, void *report);' in code
    doc = ' '.join(txt[txt.index('The REALIZE report of the n listed envs'):txt.index('int bioim_realize_report')]
                   .replace('\n *', ' ').split())
    for word in ('does not read the suspended-step flags back', 'synchronizes nothing', 'ever given an RK budget',
                 'those use bioim_osim', 'in this order', 'n == 0 returns BIOIM_OK'):
        assert word in doc, word
    _lib, L = _lib_or_skip()
    assert 'bioim_realize_report' in _lib.EXPORTS and len(L.bioim_realize_report.argtypes) == 4
    from bioimitation import packdef
    blk = C.create_string_buffer(C.sizeof(packdef.ModelPack) + 65536)
    h = C.cast(blk, C.c_void_p)
    p = C.cast(C.create_string_buffer(64), C.c_void_p)
    for msg, args in ((b'null handle', (None, -1, None, None)), (b'negative n', (h, None, -1, None)),
                      (b'null env_ids', (h, None, 1, None)), (b'null report', (h, p, 1, None)),
                      (b'null report', (h, None, 0, None))):
        a = (args[0], args[2], args[1], args[3]) if msg == b'null handle' else args
        assert L.bioim_realize_report(a[0], a[1], a[2], a[3]) == -1, msg
        assert L.bioim_last_error().startswith(b'bioim_realize_report:') and msg in L.bioim_last_error(), msg
    assert L.bioim_realize_report(h, None, 0, p) == 0
    src = open(os.path.join(REPO, 'bioimitation-gym_amd', 'csrc', 'bioim_step.hip')).read()
    body = src[src.index('int bioim_realize_report(bioim_handle_t *h'):]
    body = body[:body.index('\n}\n')]
    order = [body.index(m) for m in ('null handle', 'negative n', 'null env_ids', 'null report', 'has had an RK budget',
                                     'if (n == 0) return 0', 'hipSetDevice')]
    assert order == sorted(order) and 'bioim_pending_count' not in body and 'Synchronize' not in body
