"""Superpixel snapping of a logit map to the contours of its frame: an integer grid-SLIC on the decoded uint8 frame and the pooling of the
logits over its superpixels, on the device (``osvos_superpixels_slic`` / ``osvos_superpixels_pool``, csrc/superpixels.hip; the rule:
include/osvos_hip.h).

    assign:  a pixel takes the minimiser of (D, k), D = cell^2 dc + compactness^2 ds, over the clusters of the 3 x 3 cells around its own
    update:  a centre component becomes floor((2 sum + count) / (2 count)) over the cluster's pixels; an empty cluster keeps its centre
    pool:    every pixel of a superpixel gets the floor-divided mean of the superpixel's logits, quantised to 2^-16

The OSVOS paper snaps its masks to superpixels so that a region the image says is one piece answers as one piece; this is the cheap,
deterministic counterpart of ``refine.crf_refine``.  Integers only: the result is exact and repeats bit for bit.  There is no connectivity
enforcement (a superpixel may be disconnected; pooling does not mind) and colour is plain BGR, not CIELAB.  ``SuperpixelSnapper`` keeps its
workspaces on the device.  Nothing is read back.

The default parameters are STARTING VALUES, NOT TUNED ON DAVIS (no dataset was at hand when this was written), and no accuracy claim is
made for them: tune them on a validation split before quoting a score.
"""
import ctypes as C

import numpy as np
import torch

from ._lib import (SUPERPIXELS_MAX_CELL, SUPERPIXELS_MAX_COMPACTNESS, SUPERPIXELS_MAX_ITERS, SUPERPIXELS_MAX_K, SUPERPIXELS_MAX_SIDE, check, lib)


def check_superpixels(cell, compactness, iters):
    """ValueError unless the three parameters are integers inside the limits of osvos_superpixels_slic (host only)"""
    for name, v, lo, hi in (("cell", cell, 2, SUPERPIXELS_MAX_CELL), ("compactness", compactness, 0, SUPERPIXELS_MAX_COMPACTNESS),
                            ("iters", iters, 0, SUPERPIXELS_MAX_ITERS)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("superpixels: %s must be an integer, got %r" % (name, v))
        if not lo <= v <= hi:
            raise ValueError("superpixels: %s %d (%d..%d)" % (name, v, lo, hi))


def grid_shape(h, w, cell):
    """(GH, GW) = (ceil(h / cell), ceil(w / cell)): the cells of an h x w frame; K = GH * GW superpixels"""
    return -(-int(h) // int(cell)), -(-int(w) // int(cell))


def _need_cuda(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("osvos_pytorch_amd.superpixels needs CUDA (ROCm) tensors (%s); there is no CPU fallback" % what)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _frames(t, what):
    """[N,H,W,3] or [H,W,3] uint8 -> contiguous [N,H,W,3]"""
    _need_cuda(t, what)
    if t.dim() == 3:
        t = t[None]
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3:
        raise ValueError("%s must be a uint8 [N,H,W,3] or [H,W,3] tensor, got %s %s" % (what, t.dtype, tuple(t.shape)))
    n, h, w = (int(v) for v in t.shape[:3])
    if n < 1 or not (1 <= h <= SUPERPIXELS_MAX_SIDE and 1 <= w <= SUPERPIXELS_MAX_SIDE):
        raise ValueError("%s of %s: N >= 1 and sides 1..%d" % (what, tuple(t.shape), SUPERPIXELS_MAX_SIDE))
    return t.contiguous()


def _workspace(need, what, device, ws):
    """a uint8 CUDA tensor of at least ``need`` bytes: ``ws`` when it is large enough and on ``device``, else a new one"""
    if need == 0:
        raise ValueError("superpixels: no workspace size for %s" % what)
    if ws is None or ws.numel() < need or ws.device != device:
        ws = torch.empty(need, device=device, dtype=torch.uint8)
    return ws


def slic_workspace(n, h, w, cell, device, ws=None):
    return _workspace(int(lib().osvos_superpixels_ws_bytes(n, h, w, cell)), "%d frames of %d x %d with cell %d" % (n, h, w, cell), device, ws)


def pool_workspace(n, k, device, ws=None):
    return _workspace(int(lib().osvos_superpixels_pool_ws_bytes(n, k)), "%d frames of %d labels" % (n, k), device, ws)


def slic(frames_u8, cell=8, compactness=10, iters=5, ws=None, with_centres=False):
    """frames_u8: the decoded uint8 BGR frames [N,H,W,3] ([H,W,3] for N = 1) -> labels int32 [N,H,W] in [0, K), K = GH * GW of
    ``grid_shape``; with ``with_centres`` also centres int32 [N,K,6] = (x, y, b, g, r, count).  The frames of a batch are independent.
    Enqueued only.

    The defaults are starting values, NOT tuned on DAVIS."""
    check_superpixels(cell, compactness, iters)
    f = _frames(frames_u8, "frames_u8")
    n, h, w = (int(v) for v in f.shape[:3])
    gh, gw = grid_shape(h, w, cell)
    labels = torch.empty((n, h, w), device=f.device, dtype=torch.int32)
    centres = torch.empty((n, gh * gw, 6), device=f.device, dtype=torch.int32) if with_centres else None
    ws = slic_workspace(n, h, w, cell, f.device, ws)
    vp = C.c_void_p
    with torch.cuda.device(f.device):
        check(lib().osvos_superpixels_slic(vp(f.data_ptr()), vp(labels.data_ptr()), vp(centres.data_ptr()) if with_centres else None, vp(ws.data_ptr()),
                                           n, h, w, int(cell), int(compactness), int(iters), _stream()), "superpixels_slic")
    return (labels, centres) if with_centres else labels


def pool(logits, labels, k=None, ws=None):
    """logits: float32 CUDA tensor [N,1,H,W], [N,H,W] or [H,W]; labels: int32 [N,H,W] ([H,W] for N = 1) on the same device, ANY labelling
    -> the logits with every label's pixels replaced by the label's mean (the rule of include/osvos_hip.h: quantised to 2^-16, floor
    division), in the shape of ``logits``.  A pixel whose label is outside [0, k) keeps its logit bit for bit.  ``k`` = None takes
    labels.max() + 1, which READS BACK one number; pass k (``grid_shape``'s GH * GW for SLIC labels) to enqueue only."""
    _need_cuda(logits, "logits")
    _need_cuda(labels, "labels")
    if logits.dtype != torch.float32:
        raise ValueError("logits must be float32, got %s" % logits.dtype)
    if not (logits.dim() in (2, 3) or (logits.dim() == 4 and logits.shape[1] == 1)):
        raise ValueError("logits must be [N,1,H,W], [N,H,W] or [H,W], got %s" % (tuple(logits.shape),))
    h, w = int(logits.shape[-2]), int(logits.shape[-1])
    n = 1 if logits.dim() == 2 else int(logits.shape[0])
    if n < 1 or not (1 <= h <= SUPERPIXELS_MAX_SIDE and 1 <= w <= SUPERPIXELS_MAX_SIDE):
        raise ValueError("logits of %s: N >= 1 and sides 1..%d" % (tuple(logits.shape), SUPERPIXELS_MAX_SIDE))
    if labels.dtype != torch.int32 or labels.numel() != n * h * w or tuple(labels.shape[-2:]) != (h, w) or labels.device != logits.device:
        raise ValueError("labels must be an int32 [%d,%d,%d] tensor on the device of logits, got %s %s" % (n, h, w, labels.dtype, tuple(labels.shape)))
    if k is None:
        k = max(int(labels.max()) + 1, 1)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= SUPERPIXELS_MAX_K:
        raise ValueError("superpixels: k %r (an integer 1..%d)" % (k, SUPERPIXELS_MAX_K))
    x, lab = logits.contiguous(), labels.contiguous()
    out = torch.empty_like(x)
    ws = pool_workspace(n, int(k), x.device, ws)
    vp = C.c_void_p
    with torch.cuda.device(x.device):
        check(lib().osvos_superpixels_pool(vp(x.data_ptr()), vp(lab.data_ptr()), vp(out.data_ptr()), vp(ws.data_ptr()), n, h, w, int(k), _stream()),
              "superpixels_pool")
    return out


class SuperpixelSnapper(object):
    """Snaps logit maps to the superpixels of their frames, on the device.

    ``snapper(logits, frames_u8)`` computes the superpixels of the decoded uint8 BGR frame(s) [N,H,W,3] or [H,W,3] and returns ``logits``
    ([N,1,H,W], [N,H,W] or [H,W] float32) pooled over them, in the same shape.  ``snapper(logits, labels=labels)`` reuses labels of
    ``snapper.labels(frames_u8)`` instead (several objects over the same frames).  The workspaces stay on the device and are reused;
    enqueues only, nothing is read back.

    The defaults are starting values, NOT tuned on DAVIS."""

    def __init__(self, cell=8, compactness=10, iters=5):
        check_superpixels(cell, compactness, iters)
        self.cell, self.compactness, self.iters = int(cell), int(compactness), int(iters)
        self._ws = self._pool_ws = None

    def labels(self, frames_u8):
        """int32 [N,H,W]: the superpixels of the frames (``slic`` with this snapper's parameters and workspace)"""
        f = _frames(frames_u8, "frames_u8")
        n, h, w = (int(v) for v in f.shape[:3])
        self._ws = slic_workspace(n, h, w, self.cell, f.device, self._ws)
        return slic(f, self.cell, self.compactness, self.iters, ws=self._ws)

    def __call__(self, logits, frames_u8=None, labels=None):
        if (frames_u8 is None) == (labels is None):
            raise ValueError("SuperpixelSnapper takes the frames or their labels, one of the two")
        if labels is None:
            labels = self.labels(frames_u8)
        _need_cuda(logits, "logits")
        gh, gw = grid_shape(logits.shape[-2], logits.shape[-1], self.cell)
        n = 1 if logits.dim() == 2 else int(logits.shape[0])
        self._pool_ws = pool_workspace(n, gh * gw, logits.device, self._pool_ws)
        return pool(logits, labels, gh * gw, ws=self._pool_ws)
