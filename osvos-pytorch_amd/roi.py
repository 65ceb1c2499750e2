"""Object-centred zoom around the network: every test frame is segmented on a crop around the previous frame's mask, enlarged to one fixed
canvas, and the canvas's logits are pasted back into the frame -- all of it on the device.

``mask_box`` turns masks into boxes (``osvos_roi_box``: the tight box, a margin, a minimum size that caps the zoom, the canvas's aspect, the
clamp into the frame -- in integers; include/osvos_hip.h states the rule); ``crop_view`` resamples the box's window of the decoded uint8 frames
onto the canvas, minus the mean (``osvos_roi_view``); ``paste`` resamples the canvas's logit map onto the box's pixels and fills the rest of the
frame with a constant (``osvos_roi_paste``); ``RoiZoom`` wraps any forward callable with the three.  The box is an int32 tensor that stays on
the device: nothing is read back, and because the canvas has one size the network sees one input shape whatever the box.  Both resampling
kernels use test-time augmentation's integer-tap bilinear rule (osvos_pytorch_amd.tta), under which the full-frame box on a canvas of the
frame's size is the identity: ``RoiZoom(net.forward)`` without a previous mask, or with an empty one, is the plain forward bit for bit.

``outside`` stays a finite logit by default (-20: a probability of 2e-9), so that superpixels.pool's 2^-16 quantisation and the CRF keep
working on pasted maps.
"""
import ctypes as C
import math

import torch

from . import _glue as g
from ._lib import ROI_BOX_PARTS
from .augment import MEANVAL

MAX_SIDE = 16384          # the integer taps stay inside int32 up to here (csrc/tta_tap.h)


def _size(size, what):
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError("%s takes a size (H, W), got %r" % (what, size))
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError("%s %d x %d: every side is 1..%d" % (what, h, w, MAX_SIDE))
    return h, w


def check_zoom(margin_pct, margin_px, max_zoom):
    """ValueError unless the margins are ints >= 0 and max_zoom is a finite number >= 1"""
    g.check_int("margin_pct", margin_pct, 0, 2 ** 31 - 1, "zoom", numpy=False)
    g.check_int("margin_px", margin_px, 0, 2 ** 31 - 1, "zoom", numpy=False)
    g.check_number("max_zoom", max_zoom, 1, None, "zoom", numpy=False)


def min_size(size, canvas, max_zoom):
    """(min_h, min_w) of the box: min(side, ceil(canvas side / max_zoom)) -- a smaller box would be enlarged more than max_zoom times"""
    return tuple(min(s, int(math.ceil(c / float(max_zoom)))) for s, c in zip(size, canvas))


def _box(box, n, device):
    g.need_cuda(box, "box", "roi")
    return g.out_buffer(box, torch.int32, (n, 4), device, "the frames' device", name="box")


def full_box(n, size, device):
    """int32 [n,4] on the device: the full-frame box (0, 0, W, H) of every frame (an upload, not a read-back)"""
    h, w = _size(size, "the frame size")
    return torch.tensor([[0, 0, w, h]] * int(n), dtype=torch.int32).to(device)


def mask_box(mask, canvas, margin_pct=25, margin_px=8, max_zoom=2.0, out=None):
    """mask: bool or uint8 CUDA tensor [N,H,W], [N,1,H,W] or [H,W] (non-zero = object), canvas: (Hc, Wc) -> int32 [N,4] on the device, one
    (x0, y0, bw, bh) per frame; an empty mask gives the full frame.  out: a contiguous int32 [N,4] tensor to write into."""
    g.need_cuda(mask, "mask", "roi")
    mask, n, h, w = g.planes(mask, "mask", (torch.bool, torch.uint8))
    _size((h, w), "the mask")
    hc, wc = _size(canvas, "the canvas")
    check_zoom(margin_pct, margin_px, max_zoom)
    min_h, min_w = min_size((h, w), (hc, wc), max_zoom)
    out = torch.empty((n, 4), device=mask.device, dtype=torch.int32) if out is None else _box(out, n, mask.device)
    ws = torch.empty((n * ROI_BOX_PARTS * 4,), device=mask.device, dtype=torch.int32)      # (contents irrelevant: the call keeps no state)
    g.call("roi_box", mask.device, g.ptr(mask), g.ptr(out), n, h, w, hc, wc, margin_pct, margin_px, min_w, min_h, g.ptr(ws))
    return out


def crop_view(frames_u8, box, canvas, meanval=MEANVAL, out=None):
    """frames_u8: uint8 CUDA tensor [N,H,W,3] (BGR, as decoded), box: int32 [N,4] on the device, canvas: (Hc, Wc) -> float32 [N,3,Hc,Wc]: the
    bilinear resample of each frame's box minus meanval.  out: a contiguous float32 CUDA tensor of that shape to write into."""
    g.need_cuda(frames_u8, "frames_u8", "roi")
    frames_u8 = g.frames(frames_u8, "frames_u8", single=False)
    n, h, w = (int(v) for v in frames_u8.shape[:3])
    _box(box, n, frames_u8.device)
    hc, wc = _size(canvas, "the canvas")
    out = g.out_buffer(out, torch.float32, (n, 3, hc, wc), frames_u8.device, "the frames' device", module="roi")
    g.call("roi_view", frames_u8.device, g.ptr(frames_u8), g.ptr(box), (C.c_float * 3)(*meanval), g.ptr(out), n, h, w, hc, wc)
    return out


def paste(logits, box, size, outside=-20.0, out=None):
    """logits: float32 CUDA tensor [N,1,Hc,Wc] or [N,Hc,Wc], box: int32 [N,4] on the device, size: (H, W) of the frame -> float32 [N,1,H,W]:
    the map resampled onto each frame's box, ``outside`` elsewhere.  out: a contiguous float32 [N,1,H,W] CUDA tensor to write into."""
    g.need_cuda(logits, "logits", "roi")
    logits, n, hc, wc = g.planes(logits, "logits", (torch.float32,), dims=(3, 4))
    _box(box, n, logits.device)
    h, w = _size(size, "the frame size")
    out = g.out_buffer(out, torch.float32, (n, 1, h, w), logits.device, "the logits' device", alias=(("the logits", logits),), module="roi")
    g.call("roi_paste", logits.device, g.ptr(logits), g.ptr(box), g.ptr(out), n, hc, wc, h, w, float(outside))
    return out


class RoiZoom(object):
    """forward: any callable [N,3,h,w] -> sequence of [N,1,h,w] whose last element is the logit map (``net.forward`` fits).  Calling it with
    uint8 frames [H,W,3] or [N,H,W,3] and the previous masks (bool or uint8 [N,1,H,W], [N,H,W] or [H,W]; None: no previous mask, the
    full-frame box) returns the logits [N,1,H,W]: box -> view -> ``forward(view)[-1]`` -> paste.  canvas: (Hc, Wc) of the network's
    input, None: the frame's size.  Nothing is read back; ``self.box`` is the box tensor of the last call."""

    def __init__(self, forward, canvas=None, margin_pct=25, margin_px=8, max_zoom=2.0, outside=-20.0, meanval=MEANVAL):
        check_zoom(margin_pct, margin_px, max_zoom)
        self.forward, self.canvas = forward, None if canvas is None else _size(canvas, "the canvas")
        self.margin_pct, self.margin_px, self.max_zoom, self.outside, self.meanval = margin_pct, margin_px, max_zoom, float(outside), meanval
        self.box = None
        self._full = {}          # (N, H, W, device) -> the full-frame box tensor

    def __call__(self, frames_u8, prev_mask=None):
        g.need_cuda(frames_u8, "frames_u8", "roi")
        frames_u8 = g.frames(frames_u8, "frames_u8")
        n, h, w = (int(v) for v in frames_u8.shape[:3])
        canvas = self.canvas or (h, w)
        if prev_mask is None:
            key = (n, h, w, frames_u8.device)
            if key not in self._full:
                self._full[key] = full_box(n, (h, w), frames_u8.device)
            box = self._full[key]
        else:
            g.need_cuda(prev_mask, "prev_mask", "roi")
            if tuple(prev_mask.shape[-2:]) != (h, w) or prev_mask.numel() != n * h * w:
                raise ValueError("prev_mask %s does not fit %d frames of %d x %d" % (tuple(prev_mask.shape), n, h, w))
            box = mask_box(prev_mask.reshape(n, h, w), canvas, self.margin_pct, self.margin_px, self.max_zoom)
        view = crop_view(frames_u8, box, canvas, self.meanval)
        with torch.no_grad():
            y = self.forward(view)[-1]
        if tuple(y.shape) != (n, 1) + tuple(canvas):
            raise RuntimeError("forward returned %s for a %s batch" % (tuple(y.shape), tuple(view.shape)))
        self.box = box
        return paste(y, box, (h, w), self.outside)
