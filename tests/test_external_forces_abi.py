"""bioim_set_external_forces (include/bioim.h): the header declares it, the
binding lists it, the built library exports it, its argument checks return
BIOIM_E_ARG (-1) with a message before any device call in the header's order,
and the Python argument checks (bioimitation.external_forces) raise ValueError
without a device.  All of this runs without a GPU (the pattern of
test_ik_abi.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'bioim_set_external_forces'
ENV_ID = 'MuscleWalkingImitation2D-v0'


def _lib_or_skip():
    from bioimitation import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libbioim.so not built')
    return _lib, _lib.load()


def test_header_declares_the_call():
    txt = open(os.path.join(REPO, 'include', 'bioim.h')).read()
    code = ' '.join(re.sub(r'/\*.*?\*/', '', txt, flags=re.S).split())
    assert ('int bioim_set_external_forces(bioim_handle_t *h, int k, const int32_t *os_body , '
            'const int32_t *point_frame , const void *wrench );') in code
    assert '#define BIOIM_MAX_EXT 8' in code
    assert 'enum { BIOIM_EXT_POINT_BODY = 0, BIOIM_EXT_POINT_GROUND = 1 };' in code
    doc = txt[txt.index('Per-env external body forces ('):txt.index('#define BIOIM_MAX_EXT')]
    doc = ' '.join(doc.replace('\n *', ' ').split())
    for word in ('PrescribedForce / ExternalForce', 'fx fy fz, px py pz, tx ty tz', 'once per env at the start',
                 'held over all substeps', 'an input, not state', 'not sanitized', 'in slot order',
                 'k = 0 removes the forces', 'in this order', 'No device allocation, no synchronization'):
        assert word in doc, word


def test_binding_lists_it():
    from bioimitation import _lib
    from bioimitation import external_forces as xf
    assert NAME in _lib.EXPORTS
    assert xf.MAX_SLOTS == 8 and xf.ROW == 9 and xf.FRAMES == {'body': 0, 'ground': 1}


def test_library_exports_it():
    _lib, L = _lib_or_skip()
    assert hasattr(L, NAME)
    at = L.bioim_set_external_forces.argtypes
    assert at is not None and len(at) == 5 and at[1] is C.c_int


def test_refusals_come_before_any_device_call_in_order():
    """Each refusal of the header, in its order, on a zeroed block at least as
    large as the library's handle (the trick of test_muscle_analysis_abi.py):
    its pack has no OpenSim bodies, so a call that passes the first three
    checks ends in the fourth."""
    _lib, L = _lib_or_skip()
    from bioimitation import packdef
    blk = C.create_string_buffer(C.sizeof(packdef.ModelPack) + 65536)
    h = C.cast(blk, C.c_void_p)
    p = C.cast(C.create_string_buffer(64), C.c_void_p)
    ints = lambda *v: C.cast((C.c_int32 * len(v))(*v), C.c_void_p)  # noqa: E731

    def refused(msg, *args):
        assert L.bioim_set_external_forces(*args) == -1, msg
        err = L.bioim_last_error()
        assert err.startswith(b'bioim_set_external_forces:') and msg in err, (msg, err)
    refused(b'null handle', None, 1, p, p, p)
    refused(b'null handle', None, -1, None, None, None)
    for k in (-1, 9, 1 << 20):
        refused(b'k must be in [0, BIOIM_MAX_EXT]', h, k, None, None, None)
    for arrs in ((None, p, p), (p, None, p), (p, p, None)):
        refused(b'null os_body, point_frame or wrench', h, 8, *arrs)
    refused(b'no OpenSim body 0', h, 1, ints(0), ints(7), p)          # the zeroed pack has none; the bad frame comes later
    refused(b'no OpenSim body -1', h, 2, ints(-1, 0), ints(0, 0), p)
    # k = 0 on a handle without forces: nothing to do, no device call
    assert L.bioim_set_external_forces(h, 0, None, None, None) == 0
    src = open(os.path.join(REPO, 'bioimitation-gym_amd', 'csrc', 'bioim_step.hip')).read()
    body = src[src.index('int bioim_set_external_forces(bioim_handle_t *h'):]
    body = body[:body.index('\n}\n')]
    order = [body.index(m) for m in ('null handle', 'k must be in', 'null os_body', 'no OpenSim body',
                                     'point_frame must be', 'a perturbation table is set',
                                     'the semi-implicit integrator only', 'hipSetDevice')]
    assert order == sorted(order)
    assert 'hipMalloc' not in body and 'Synchronize' not in body
    # the other setters refuse the second call too
    for fn, msg in (('bioim_set_perturbation', 'external forces are set'), ('bioim_set_integrator', 'external forces are set'),
                    ('bioim_set_rk_budget', 'external forces are set')):
        b = src[src.index(f'int {fn}(bioim_handle_t *h'):]
        b = b[:b.index('\n}\n')]
        assert msg in b and 'h->ext_k > 0' in b, fn
        assert b.index(msg) < (b.index('hip') if 'hip' in b else len(b)), fn


def test_slot_checks_need_no_device():
    from bioimitation import external_forces as xf
    from bioimitation.obslayout import load_names
    bodies = list(load_names(ENV_ID)['bodies'])
    body, frame = xf.check_slots(bodies, ['torso', 'calcn_r', 'torso'], ['body', 'ground', 'body'])
    assert body.dtype == np.int32 and frame.dtype == np.int32
    assert list(body) == [bodies.index('torso'), bodies.index('calcn_r'), bodies.index('torso')]
    assert list(frame) == [0, 1, 0]
    assert list(xf.check_slots(bodies, ['torso'] * 8, 'ground')[1]) == [1] * 8
    assert list(xf.check_slots(bodies, 'torso')[0]) == [bodies.index('torso')]
    bad = [
        (dict(points=['humerus_r']), 'unknown body'),
        (dict(points=['torso', 3]), 'unknown body'),
        (dict(points=['torso'] * 9), 'at most 8'),
        (dict(points=[]), 'no slots'),
        (dict(points=5), 'sequence of body names'),
        (dict(points=['torso'], point_in='world'), 'point_in must be one of'),
        (dict(points=['torso', 'torso'], point_in=['body']), 'point_in has 1 entries for 2 slots'),
        (dict(points=['torso'], point_in=[0]), 'point_in must be one of'),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            xf.check_slots(bodies, **kw)


def test_wrench_checks_need_no_device():
    torch = pytest.importorskip('torch')
    from bioimitation import external_forces as xf
    n, k = 4, 3
    cpu, gpu = torch.device('cpu'), torch.device('cuda', 0)
    w = torch.zeros((n, k, 9), dtype=torch.float64)
    assert xf.check_wrench(w, n, k, torch.float64, cpu) is w
    bad = [
        (np.zeros((n, k, 9)), torch.float64, cpu, 'must be a torch tensor'),
        (torch.zeros((n, k, 6), dtype=torch.float64), torch.float64, cpu, 'contiguous'),
        (torch.zeros((n, k + 1, 9), dtype=torch.float64), torch.float64, cpu, 'contiguous'),
        (torch.zeros((n * k, 9), dtype=torch.float64), torch.float64, cpu, 'contiguous'),
        (torch.zeros((n, k, 9), dtype=torch.float32), torch.float64, cpu, 'torch.float64'),
        (w, torch.float32, cpu, 'torch.float32'),
        (w, torch.float64, gpu, 'on cuda:0'),
        (torch.zeros((n, k, 18), dtype=torch.float64)[:, :, ::2], torch.float64, cpu, 'not contiguous'),
        (torch.zeros((k, n, 9), dtype=torch.float64).transpose(0, 1), torch.float64, cpu, 'not contiguous'),
    ]
    for t, dtype, dev, msg in bad:
        with pytest.raises(ValueError, match=msg):
            xf.check_wrench(t, n, k, dtype, dev)


def test_forces_exclude_a_push_and_rk():
    """Whichever comes second is refused: the check VectorEnv.set_external_forces
    makes before the library call, and the source of the methods that come
    second the other way round."""
    from bioimitation import external_forces as xf
    xf.check_compatible(None, 'semi-implicit', 0)
    with pytest.raises(ValueError, match='apply_perturbations'):
        xf.check_compatible((np.zeros(2), np.zeros((1, 2))), 'semi-implicit')
    with pytest.raises(ValueError, match="integrator='semi-implicit' only"):
        xf.check_compatible(None, 'rk-merson')
    with pytest.raises(ValueError, match='with an RK budget'):
        xf.check_compatible(None, 'rk-merson', 4)
    import inspect
    from bioimitation.vector_env import MixedVectorEnv, VectorEnv
    src = inspect.getsource(VectorEnv.set_external_forces)
    assert src.index('check_slots') < src.index('check_compatible') < src.index('check_wrench') \
        < src.index('bioim_set_external_forces(self._h, k')
    for meth in (VectorEnv.set_perturbation, VectorEnv.set_rk_budget):
        s = inspect.getsource(meth)
        assert 'external forces are set' in s and s.index('external forces are set') < s.index('_lib.check')
    assert hasattr(VectorEnv, 'external_wrench_ground') and hasattr(MixedVectorEnv, 'set_external_forces')
    import bioimitation.envs as envs
    assert any(hasattr(c, 'set_external_forces') for c in vars(envs).values() if inspect.isclass(c))


def test_wrench_ground_is_the_analyses_ext():
    """force, point x force + torque, summed per composite body (CPU tensors)."""
    torch = pytest.importorskip('torch')
    from bioimitation import external_forces as xf
    rng = np.random.default_rng(0)
    n, nos, ncb = 3, 4, 3
    cbody = [0, 1, 1, 2]
    w = torch.as_tensor(rng.normal(size=(n, 3, 9)))
    origin = torch.as_tensor(rng.normal(size=(n, nos, 3)))
    A = rng.normal(size=(n, nos, 3, 3))
    rot = torch.as_tensor(np.linalg.qr(A)[0].reshape(n, nos, 9))
    body, frame = np.array([1, 2, 3], dtype=np.int32), np.array([0, 0, 1], dtype=np.int32)
    ext = xf.wrench_ground(w, body, frame, cbody, ncb, origin, rot).numpy()
    ref = np.zeros((n, ncb, 6))
    for i in range(n):
        for j in range(3):
            f, p, t = (w[i, j, 3 * a:3 * a + 3].numpy() for a in range(3))
            b = int(body[j])
            P = p if frame[j] else origin[i, b].numpy() + rot[i, b].numpy().reshape(3, 3) @ p
            ref[i, cbody[b], :3] += f
            ref[i, cbody[b], 3:] += np.cross(P, f) + t
    assert not ext[:, 0].any()
    assert np.allclose(ext, ref, rtol=0, atol=1e-13)


def test_hazard_gate_scans_the_kernels():
    import sys
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import hazard_gate
    assert any(k in '_Z14env_kernel_extI' for k in hazard_gate.KERNELS)
