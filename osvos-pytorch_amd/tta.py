"""Test-time augmentation around the network: every frame runs at several scales and mirrored, the views' logit maps are brought back to
the frame's grid and averaged -- all of it on the device.

``make_view`` makes one resized (and optionally mirrored) mean-subtracted network input from the decoded uint8 frames (``osvos_tta_view``);
``fuse_views`` resamples V logit maps of different sizes onto one grid, un-mirrors them and sums them with their weights in one pass
(``osvos_tta_fuse``); ``TestTimeAugment`` wraps any forward callable with the two.  Both kernels sample with the same integer-tap bilinear rule
(half-pixel centres, the geometry of ``F.interpolate(mode='bilinear', align_corners=False)``; include/osvos_hip.h), under which a view of the
frame's own size passes through bit for bit: ``TestTimeAugment(net.forward)`` with the default single scale is the plain forward.

LOGITS are averaged, never sigmoids: everything downstream (``results.save_masks``, the evaluators, ``ComponentTracker``, ``merge_objects``)
takes logits, and the logit of a mean probability saturates in fp32.
"""
import ctypes as C
import math

import torch

from . import _glue as g
from ._lib import TTA_MAX_VIEWS, ptr_array
from .augment import MEANVAL

MAX_SIDE = 16384          # the integer taps stay inside int32 up to here (csrc/tta.hip)


def view_size(h, w, s):
    """size of the view of an h x w frame at scale s: max(1, floor(side * s + 0.5)) per side"""
    s = float(s)
    if not (s > 0.0 and math.isfinite(s)):
        raise ValueError("a test-time augmentation scale must be a positive number, got %r" % (s,))
    return max(1, int(math.floor(h * s + 0.5))), max(1, int(math.floor(w * s + 0.5)))


def plan(h, w, scales, flip):
    """[(hv, wv, flipped)] in call order: the scales in the given order, for each the plain view first, then the mirrored one"""
    scales = tuple(scales)
    if not scales:
        raise ValueError("test-time augmentation needs at least one scale")
    sizes = [view_size(h, w, s) for s in scales]
    for (hv, wv), s in zip(sizes, scales):
        if hv > MAX_SIDE or wv > MAX_SIDE:
            raise ValueError("scale %g makes a %d x %d view of a %d x %d frame (at most %d per side)" % (s, hv, wv, h, w, MAX_SIDE))
    if len(set(sizes)) != len(sizes):
        raise ValueError("scales %s give the same view size twice on a %d x %d frame: %s" % (list(scales), h, w, sizes))
    if len(sizes) * (2 if flip else 1) > TTA_MAX_VIEWS:
        raise ValueError("%d scales%s make %d views (at most %d)" % (len(sizes), " with flip" if flip else "", len(sizes) * (2 if flip else 1),
                                                                    TTA_MAX_VIEWS))
    out = []
    for hv, wv in sizes:
        out.append((hv, wv, False))
        if flip:
            out.append((hv, wv, True))
    return out


def parse_scales(text):
    """'0.75,1,1.25' -> (0.75, 1.0, 1.25); '' -> (); ValueError on anything that is not a list of positive numbers"""
    out = []
    for t in (text or "").split(","):
        if not t.strip():
            continue
        try:
            out.append(float(t))
        except ValueError:
            raise ValueError("%r is not a number" % t.strip())
        view_size(1, 1, out[-1])
    return tuple(out)


def make_view(frames_u8, hv, wv, flip=False, meanval=MEANVAL, out=None):
    """frames_u8: uint8 CUDA tensor [N,H,W,3] (BGR, as decoded) -> float32 [N,3,hv,wv]: bilinear resample minus meanval, mirrored when flip.
    out: a contiguous float32 CUDA tensor of that shape to write into (e.g. one half of a batch)."""
    g.need_cuda(frames_u8, "frames_u8", "tta")
    frames_u8 = g.frames(frames_u8, "frames_u8", single=False)
    n, h, w = (int(v) for v in frames_u8.shape[:3])
    hv, wv = int(hv), int(wv)
    out = g.out_buffer(out, torch.float32, (n, 3, hv, wv), frames_u8.device, "the frames' device", module="tta")
    g.call("tta_view", frames_u8.device, g.ptr(frames_u8), (C.c_float * 3)(*meanval), g.ptr(out), n, h, w, hv, wv, int(bool(flip)))
    return out


def fuse_views(views, flips, size, weights=None, out=None):
    """views: V float32 CUDA tensors [N,1,hv,wv] or [N,hv,wv] (logits; sizes may differ), flips: V bools (the view came from a mirrored
    input), size: (H, W) of the grid, weights: V floats or None (1 / V each) -> float32 [N,1,H,W] = sum_v weights[v] * resampled view v."""
    views = list(views)
    flips = [bool(f) for f in flips]
    if not 1 <= len(views) <= TTA_MAX_VIEWS:
        raise ValueError("fuse_views takes 1..%d views, got %d" % (TTA_MAX_VIEWS, len(views)))
    if len(flips) != len(views) or (weights is not None and len(weights) != len(views)):
        raise ValueError("fuse_views: one flip flag (and one weight) per view")
    keep, hvs, wvs, n = [], [], [], None
    for v in views:
        g.need_cuda(v, "views", "tta")
        v, nv, hv, wv = g.planes(v, "every view", (torch.float32,), dims=(3, 4))
        if n is None:
            n = nv
        if nv != n or v.device != views[0].device:
            raise ValueError("the views must share the batch size and the device")
        keep.append(v)
        hvs.append(hv)
        wvs.append(wv)
    h, w = int(size[0]), int(size[1])
    out = g.out_buffer(out, torch.float32, (n, 1, h, w), keep[0].device, "the views' device", module="tta")
    V = len(keep)
    ia = C.c_int * V
    wt = (C.c_float * V)(*[float(x) for x in weights]) if weights is not None else None
    g.call("tta_fuse", keep[0].device, ptr_array([v.data_ptr() for v in keep]), ia(*hvs), ia(*wvs), ia(*[int(f) for f in flips]), wt, V, g.ptr(out),
           n, h, w)
    return out


class TestTimeAugment(object):
    """forward: any callable [N,3,h,w] -> sequence of [N,1,h,w] whose last element is the map to fuse (``net.forward`` fits).  Calling it
    with uint8 frames [H,W,3] or [N,H,W,3] returns the fused logits [N,1,H,W]: per scale one batch holding the plain view and (flip) the
    mirrored one, one forward call per scale, one fuse over all views.  Nothing is read back."""
    __test__ = False          # (the name starts with Test: not a test class)

    def __init__(self, forward, scales=(1.0,), flip=False, weights=None, meanval=MEANVAL):
        self.forward, self.scales, self.flip, self.meanval = forward, tuple(float(s) for s in scales), bool(flip), meanval
        if not self.scales:
            raise ValueError("test-time augmentation needs at least one scale")
        for s in self.scales:
            view_size(1, 1, s)                              # (positive and finite; the sizes are checked per frame size by plan)
        views = len(self.scales) * (2 if self.flip else 1)
        if views > TTA_MAX_VIEWS:
            raise ValueError("%d scales%s make %d views (at most %d)" % (len(self.scales), " with flip" if self.flip else "", views, TTA_MAX_VIEWS))
        if weights is not None and len(weights) != views:
            raise ValueError("%d weights for %d views" % (len(weights), views))
        self.weights = None if weights is None else [float(x) for x in weights]

    def __call__(self, frames_u8, return_views=False):
        g.need_cuda(frames_u8, "frames_u8", "tta")
        frames_u8 = g.frames(frames_u8, "frames_u8")
        n, h, w = (int(v) for v in frames_u8.shape[:3])
        p = plan(h, w, self.scales, self.flip)
        per = 2 if self.flip else 1
        maps = []
        for i in range(len(self.scales)):
            hv, wv, _ = p[i * per]
            batch = torch.empty((per * n, 3, hv, wv), device=frames_u8.device, dtype=torch.float32)
            for k in range(per):
                make_view(frames_u8, hv, wv, flip=p[i * per + k][2], meanval=self.meanval, out=batch[k * n:(k + 1) * n])
            with torch.no_grad():
                y = self.forward(batch)[-1]
            if tuple(y.shape) != (per * n, 1, hv, wv):
                raise RuntimeError("forward returned %s for a %s batch" % (tuple(y.shape), tuple(batch.shape)))
            maps += [y[k * n:(k + 1) * n] for k in range(per)]
        fused = fuse_views(maps, [f for _, _, f in p], (h, w), self.weights)
        return (fused, maps, p) if return_views else fused
