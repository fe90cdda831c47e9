"""What the batched analyses share on the Python side (``inverse_dynamics``,
``muscle_analysis``, ``static_optimization``, ``inverse_kinematics``,
``joint_reaction``, ``induced_accelerations``): the argument checks that
need no device, the move of an input to the env's device, and the 1-env
``VectorEnv`` an analysis object owns.  ``name`` is the analysis's own name,
the prefix of its error messages ('muscle analysis', ...)."""
from __future__ import annotations

import ctypes as C

import numpy as np


def dtype_kind(x):
    """numpy's kind letter of an array's or a tensor's dtype: 'f', 'i', 'u',
    'b' or 'c' (a torch integer dtype, signed or not, is 'i')."""
    dt = x.dtype
    if isinstance(dt, np.dtype):
        return dt.kind
    if dt.is_floating_point:      # a torch dtype
        return 'f'
    return 'c' if dt.is_complex else ('b' if 'bool' in str(dt) else 'i')


def _shape_text(dims):
    return f'({dims[0]},)' if len(dims) == 1 else f'({", ".join(map(str, dims))})'


def check_shape(name, x, what, tail, batched=True, kinds='fiu'):
    """``x`` (array, tensor or nested list) holds real numbers (a dtype kind
    in ``kinds``) and has shape ``(n,) + tail`` (``tail`` alone when not
    ``batched``).  Returns its shape."""
    if not hasattr(x, 'dtype') or not hasattr(x, 'shape'):
        try:
            x = np.asarray(x)
        except (TypeError, ValueError):
            raise ValueError(f'{name}: {what} must hold real numbers') from None
    if dtype_kind(x) not in kinds:
        raise ValueError(f'{name}: {what} must hold real numbers, got dtype {x.dtype}')
    s, tail = tuple(x.shape), tuple(tail)
    if len(s) != batched + len(tail) or s[batched:] != tail:
        raise ValueError(f'{name}: {what} must have shape {_shape_text((("n",) if batched else ()) + tail)}, got {s}')
    return s


def check_rows(name, first, others, unit=''):
    """The row count n of ``first`` = (x, what, tail), which every given
    (not None) entry of ``others`` = (x, what, tail[, kinds]) must share."""
    n = check_shape(name, *first)[0]
    for x, what, tail, *kinds in others:
        if x is not None:
            nx = check_shape(name, x, what, tail, True, *kinds)[0]
            if nx != n:
                raise ValueError(f'{name}: {what} has {nx} rows, {first[1]} has {n}{unit}')
    return n


def check_want(name, want, keys):
    """``want`` (a key or a sequence of keys of ``keys``) as a tuple."""
    if isinstance(want, str):
        want = (want,)
    want = tuple(want)
    if not want:
        raise ValueError(f'{name}: nothing requested (want is empty)')
    for k in want:
        if k not in keys:
            raise ValueError(f'{name}: unknown key {k!r}; choose from {keys}')
    return want


def check_reserve(name, reserve, ndof):
    """The row weights λ = 1/reserve² as a float64 array ``[ndof]``.
    ``reserve``: a scalar or ``[ndof]`` of positive numbers, N·m, ``inf``
    allowed (λ = 0 leaves the row out)."""
    if hasattr(reserve, 'detach'):    # a torch tensor
        reserve = reserve.detach().cpu().numpy()
    try:
        r = np.asarray(reserve, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f'{name}: reserve must hold real numbers') from None
    if r.shape not in ((), (ndof,)):
        raise ValueError(f'{name}: reserve must be a scalar or have shape ({ndof},), got {r.shape}')
    if np.isnan(r).any() or (r < 0).any():
        raise ValueError(f'{name}: reserve must be non-negative (inf allowed), not NaN')
    if (r == 0).any():
        raise ValueError(f'{name}: a reserve of 0 N·m has no finite weight; use a small positive value')
    return np.broadcast_to(1.0 / (r * r), (ndof,)).copy()


def to_device(x, device, dtype):
    """``x`` (None, array, tensor or nested list) as a contiguous tensor of
    ``dtype`` on ``device``."""
    import torch
    if x is None:
        return None
    if isinstance(x, np.ndarray) and not x.flags.writeable:
        x = x.copy()      # torch does not wrap read-only arrays
    return torch.as_tensor(x).to(device=device, dtype=dtype).contiguous()


def ptr(t):
    """A tensor's device pointer for a ``void *`` argument (None: null)."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Analysis:
    """An analysis object's own 1-env ``VectorEnv`` (the model image and the
    stream its launches run on), with its ``device`` and ``dtype``."""

    def __init__(self, env_id: str, device: int = 0, precision: int = 64):
        from .vector_env import VectorEnv
        self._env = VectorEnv(env_id, 1, device=device, precision=precision)
        self.device, self.dtype = self._env.device, self._env.dtype

    def _dev(self, x, dtype=None):
        return to_device(x, self.device, dtype or self.dtype)

    def close(self):
        self._env.close()
