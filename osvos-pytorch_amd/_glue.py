"""The plumbing between a torch tensor and the C ABI (include/osvos_hip.h) that every stage wrapper needs, written once: the device-guarded
library call, the CUDA refusal, the shape rules of frames, planes and ``out=`` buffers, the number checks, the workspace rule and the
option-list parser.  Functions only.  The shape rules and checks read shape, dtype and device alone, so they run on CPU tensors
(tests/test_glue_cpu.py); ``need_cuda`` is the separate first step of a wrapper.
"""
import ctypes as C
import math

import numpy as np
import torch

from ._lib import check, lib


def stream():
    """the current stream of the current device, as the C ABI takes it"""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def call(name, device, *args):
    """``osvos_<name>(*args, stream)`` on ``device``, whatever the caller's current device is: the call is made with ``device`` current, so
    the stream it gets is that device's.  Every stage entry point takes the stream last.  (The guard costs about 2 us of host time, as much
    again as the rest of a wrapper: it is entered only when ``device`` is not the current one already.)"""
    fn = getattr(lib(), "osvos_" + name)
    if device.index == torch.cuda.current_device():
        check(fn(*args, stream()), name)
    else:
        with torch.cuda.device(device):
            check(fn(*args, stream()), name)


def need_cuda(t, what, module):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("osvos_pytorch_amd.%s needs CUDA (ROCm) tensors (%s); there is no CPU fallback" % (module, what))


def _name(dtype):
    return str(dtype).replace("torch.", "")


def frames(t, what, max_side=None, single=True, batch=True):
    """the decoded frames: uint8 [N,H,W,3] (``batch``) or [H,W,3] (``single``) -> contiguous [N,H,W,3]; with ``max_side`` also N >= 1 and
    sides 1..max_side"""
    if t.dtype != torch.uint8 or t.shape[-1:] != (3,) or not ((batch and t.dim() == 4) or (single and t.dim() == 3)):
        raise ValueError("%s must be a uint8 %s tensor, got %s %s" % (what, " or ".join(["[N,H,W,3]"] * batch + ["[H,W,3]"] * single), t.dtype,
                                                                   tuple(t.shape)))
    if t.dim() == 3:
        t = t[None]
    if max_side is not None and (t.shape[0] < 1 or not (1 <= t.shape[1] <= max_side and 1 <= t.shape[2] <= max_side)):
        raise ValueError("%s of %s: N >= 1 and sides 1..%d" % (what, tuple(t.shape), max_side))
    return t.contiguous()


def planes(t, what, dtypes=None, max_side=None, dims=(2, 3, 4)):
    """a stack of planes [N,1,H,W], [N,H,W] or [H,W] (those of ``dims``) of one of ``dtypes`` (None: any) -> (the contiguous tensor in its
    own shape, N, H, W); with ``max_side`` also N >= 1 and sides 1..max_side"""
    shapes = {2: "[H,W]", 3: "[N,H,W]", 4: "[N,1,H,W]"}
    if (dtypes is not None and t.dtype not in dtypes) or t.dim() not in dims or (t.dim() == 4 and t.shape[1] != 1):
        raise ValueError("%s must be a %s tensor of shape %s, got %s %s" % (what, "any" if dtypes is None else ", ".join(_name(d) for d in dtypes),
                                                                         " or ".join(shapes[d] for d in sorted(dims, reverse=True)), t.dtype,
                                                                         tuple(t.shape)))
    n, h, w = 1 if t.dim() == 2 else int(t.shape[0]), int(t.shape[-2]), int(t.shape[-1])
    if max_side is not None and (n < 1 or not (1 <= h <= max_side and 1 <= w <= max_side)):
        raise ValueError("%s of %s: N >= 1 and sides 1..%d" % (what, tuple(t.shape), max_side))
    return t.contiguous(), n, h, w


def out_buffer(out, dtype, shape, device, where, alias=(), name="out", module=None):
    """the tensor a wrapper writes into: a new one when ``out`` is None, else the caller's after its check -- contiguous, of ``dtype`` and
    ``shape``, on ``device`` (``where`` says whose, e.g. "the frames' device"), and starting where none of ``alias`` -- (name, tensor or
    None) pairs -- starts.  With ``module`` the caller's tensor passes ``need_cuda`` first."""
    if out is None:
        return torch.empty(tuple(shape), device=device, dtype=dtype)
    if module is not None:
        need_cuda(out, name, module)
    if out.dtype != dtype or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != device:
        raise ValueError("%s must be a contiguous %s %s tensor on %s" % (name, _name(dtype), list(shape), where))
    for other, t in alias:
        if t is not None and out.data_ptr() == t.data_ptr():
            raise ValueError("%s must not be %s" % (name, other))
    return out


def check_int(name, v, lo, hi, prefix, numpy=True):
    """ValueError unless ``v`` is an integer (never a bool; numpy's integers with ``numpy``) in lo..hi (hi None: no upper limit)"""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer) if numpy else int):
        raise ValueError("%s: %s must be an integer, got %r" % (prefix, name, v))
    if v < lo or (hi is not None and v > hi):
        raise ValueError("%s: %s %d (%s)" % (prefix, name, v, ">= %d" % lo if hi is None else "%d..%d" % (lo, hi)))


def check_number(name, v, lo, hi, prefix, numpy=True):
    """ValueError unless ``v`` is a finite number (never a bool; numpy's scalars with ``numpy``) in lo..hi (hi None: no upper limit)"""
    kinds = (int, float, np.integer, np.floating) if numpy else (int, float)
    if isinstance(v, bool) or not isinstance(v, kinds) or not math.isfinite(v) or v < lo or (hi is not None and v > hi):
        raise ValueError("%s: %s %r (a finite number %s)" % (prefix, name, v, ">= %g" % lo if hi is None else "in %g..%g" % (lo, hi)))


def grid_shape(h, w, cell):
    """(GH, GW) = (ceil(h / cell), ceil(w / cell)): the cells of an h x w frame"""
    return -(-int(h) // int(cell)), -(-int(w) // int(cell))


def workspace(need_bytes, device, ws=None, what="", prefix="", dtype=torch.uint8, align=1):
    """a tensor of at least ``need_bytes`` bytes on ``device``: ``ws`` itself when it is one, is large enough (in bytes, whatever its dtype)
    and starts on a multiple of ``align``, else a new one of ``dtype``.  ValueError when the library answered 0: it has no size for the call."""
    need = int(need_bytes)
    if need == 0:
        raise ValueError("%s: no workspace size for %s" % (prefix, what))
    if not isinstance(ws, torch.Tensor) or ws.device != device or ws.numel() * ws.element_size() < need or ws.data_ptr() % align:
        ws = torch.empty(-(-need // dtype.itemsize), device=device, dtype=dtype)
    return ws


def parse_numbers(text, kinds, what, sep=",", expect=None, finite=False):
    """'0.25,0.05', '25,8' or (sep 'x'; 'X' too) '240x427' -> one value per kind of ``kinds`` (int or float), a tuple.  ValueError
    "<what> takes <expect>, got <text>" on another count or a part that is no such number; with ``finite`` also on inf and nan"""
    parts = (text or "").lower().split(sep)
    expect = expect or "%d comma-separated numbers" % len(kinds)
    try:
        vals = tuple(kind(v) for kind, v in zip(kinds, parts)) if len(parts) == len(kinds) else None
    except ValueError:
        vals = None
    if vals is None:
        raise ValueError("%s takes %s, got %r" % (what, expect, text))
    if finite and not all(math.isfinite(v) for v in vals):
        raise ValueError("%s takes finite numbers, got %r" % (what, text))
    return vals
