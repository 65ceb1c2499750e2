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
import torch

from . import _glue as g
from ._glue import grid_shape  # noqa: F401  (superpixels.grid_shape: the cells of a frame; K = GH * GW superpixels)
from ._lib import (SUPERPIXELS_MAX_CELL, SUPERPIXELS_MAX_COMPACTNESS, SUPERPIXELS_MAX_ITERS, SUPERPIXELS_MAX_K, SUPERPIXELS_MAX_SIDE, lib)


def check_superpixels(cell, compactness, iters):
    """ValueError unless the three parameters are integers inside the limits of osvos_superpixels_slic (host only)"""
    for name, v, lo, hi in (("cell", cell, 2, SUPERPIXELS_MAX_CELL), ("compactness", compactness, 0, SUPERPIXELS_MAX_COMPACTNESS),
                            ("iters", iters, 0, SUPERPIXELS_MAX_ITERS)):
        g.check_int(name, v, lo, hi, "superpixels")


def _frames(t, what):
    """[N,H,W,3] or [H,W,3] uint8 -> contiguous [N,H,W,3]"""
    g.need_cuda(t, what, "superpixels")
    return g.frames(t, what, SUPERPIXELS_MAX_SIDE)


def slic_workspace(n, h, w, cell, device, ws=None):
    return g.workspace(lib().osvos_superpixels_ws_bytes(n, h, w, cell), device, ws, "%d frames of %d x %d with cell %d" % (n, h, w, cell),
                       "superpixels")


def pool_workspace(n, k, device, ws=None):
    return g.workspace(lib().osvos_superpixels_pool_ws_bytes(n, k), device, ws, "%d frames of %d labels" % (n, k), "superpixels")


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
    g.call("superpixels_slic", f.device, g.ptr(f), g.ptr(labels), g.ptr(centres), g.ptr(ws), n, h, w, int(cell), int(compactness), int(iters))
    return (labels, centres) if with_centres else labels


def pool(logits, labels, k=None, ws=None):
    """logits: float32 CUDA tensor [N,1,H,W], [N,H,W] or [H,W]; labels: int32 [N,H,W] ([H,W] for N = 1) on the same device, ANY labelling
    -> the logits with every label's pixels replaced by the label's mean (the rule of include/osvos_hip.h: quantised to 2^-16, floor
    division), in the shape of ``logits``.  A pixel whose label is outside [0, k) keeps its logit bit for bit.  ``k`` = None takes
    labels.max() + 1, which READS BACK one number; pass k (``grid_shape``'s GH * GW for SLIC labels) to enqueue only."""
    g.need_cuda(logits, "logits", "superpixels")
    g.need_cuda(labels, "labels", "superpixels")
    x, n, h, w = g.planes(logits, "logits", (torch.float32,), SUPERPIXELS_MAX_SIDE)
    if labels.dtype != torch.int32 or labels.numel() != n * h * w or tuple(labels.shape[-2:]) != (h, w) or labels.device != logits.device:
        raise ValueError("labels must be an int32 [%d,%d,%d] tensor on the device of logits, got %s %s" % (n, h, w, labels.dtype, tuple(labels.shape)))
    if k is None:
        k = max(int(labels.max()) + 1, 1)
    g.check_int("k", k, 1, SUPERPIXELS_MAX_K, "superpixels")
    lab = labels.contiguous()
    out = torch.empty_like(x)
    ws = pool_workspace(n, int(k), x.device, ws)
    g.call("superpixels_pool", x.device, g.ptr(x), g.ptr(lab), g.ptr(out), g.ptr(ws), n, h, w, int(k))
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
        g.need_cuda(logits, "logits", "superpixels")
        gh, gw = grid_shape(logits.shape[-2], logits.shape[-1], self.cell)
        n = 1 if logits.dim() == 2 else int(logits.shape[0])
        self._pool_ws = pool_workspace(n, gh * gw, logits.device, self._pool_ws)
        return pool(logits, labels, gh * gw, ws=self._pool_ws)
