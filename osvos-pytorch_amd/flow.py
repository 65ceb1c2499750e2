"""Motion compensation of what the test loop carries from frame t-1 to frame t: a block-matching motion field between two decoded frames
and the integer warp that applies it, on the device (``osvos_flow_block_match`` / ``osvos_flow_warp``, csrc/flow.hip; the rule:
include/osvos_hip.h).

    cost(d) = sum over the cell's block of |Ycur(clamp(p)) - Yprev(clamp(p + d))| + penalty (|dx| + |dy|),   |dx|, |dy| <= search

One vector per ``step`` x ``step`` cell, the minimiser of (cost, dx^2 + dy^2, dy, dx) over a ``block`` x ``block`` square centred on the
cell, ``median`` 3 x 3 median passes over the vector grid.  The field is BACKWARD: it points from a pixel of the current frame to where it
was in the previous one, so ``warp(prev_mask, vec, step)`` is the previous mask in the current frame's coordinates.  Integers only: the
result is exact and the warp is a gather (bytes, and float32 bit for bit).  ``MotionCompensator`` keeps the previous frame and the
workspace on the device; its output goes to ``adapt.OnlineAdapter`` (the previous mask) and ``results.ComponentTracker.seed``.  Nothing is
read back.

The default parameters are STARTING VALUES, NOT TUNED ON DAVIS (no dataset was at hand when this was written), and no accuracy claim is
made for them: tune them on a validation split before quoting a score.
"""
import torch

from . import _glue as g
from ._glue import grid_shape  # noqa: F401  (flow.grid_shape: the cells of a frame at a grid step)
from ._lib import (FLOW_MAX_BLOCK, FLOW_MAX_MEDIAN, FLOW_MAX_PENALTY, FLOW_MAX_SEARCH, FLOW_MAX_SIDE, FLOW_MAX_STEP, lib)


def check_flow(search, block, step, penalty, median):
    """ValueError unless the five parameters are integers inside the limits of osvos_flow_block_match (host only)"""
    for name, v, lo, hi in (("search", search, 0, FLOW_MAX_SEARCH), ("block", block, 1, FLOW_MAX_BLOCK), ("step", step, 1, FLOW_MAX_STEP),
                            ("penalty", penalty, 0, FLOW_MAX_PENALTY), ("median", median, 0, FLOW_MAX_MEDIAN)):
        g.check_int(name, v, lo, hi, "flow")


def _frames(t, what):
    """[N,H,W,3] or [H,W,3] uint8 -> contiguous [N,H,W,3]"""
    g.need_cuda(t, what, "flow")
    return g.frames(t, what, FLOW_MAX_SIDE)


def workspace(n, h, w, block, step, search, median, device, ws=None):
    """a uint8 CUDA tensor of at least osvos_flow_ws_bytes bytes: ``ws`` when it is large enough and on ``device``, else a new one"""
    return g.workspace(lib().osvos_flow_ws_bytes(n, h, w, block, step, search, median), device, ws,
                       "%d frames of %d x %d with block %d step %d search %d median %d" % (n, h, w, block, step, search, median), "flow")


def block_match(prev_u8, cur_u8, search=24, block=16, step=4, penalty=4, median=1, ws=None):
    """prev_u8, cur_u8: the decoded uint8 BGR frames [N,H,W,3] ([H,W,3] for N = 1) on one device -> (vec int32 [N,GH,GW,2] = (dx, dy) per
    cell, cost int32 [N,GH,GW] = the cell's minimal cost before the median passes).  Frame n of ``cur_u8`` is matched against frame n of
    ``prev_u8``; the frames of a batch are independent.  Enqueued only.

    The defaults are starting values, NOT tuned on DAVIS."""
    check_flow(search, block, step, penalty, median)
    p, c = _frames(prev_u8, "prev_u8"), _frames(cur_u8, "cur_u8")
    if p.shape != c.shape or p.device != c.device:
        raise ValueError("prev_u8 %s and cur_u8 %s must have one shape and one device" % (tuple(p.shape), tuple(c.shape)))
    n, h, w = (int(v) for v in c.shape[:3])
    gh, gw = grid_shape(h, w, step)
    vec = torch.empty((n, gh, gw, 2), device=c.device, dtype=torch.int32)
    cost = torch.empty((n, gh, gw), device=c.device, dtype=torch.int32)
    ws = workspace(n, h, w, block, step, search, median, c.device, ws)
    g.call("flow_block_match", c.device, g.ptr(p), g.ptr(c), g.ptr(vec), g.ptr(cost), g.ptr(ws), n, h, w, int(block), int(step), int(search),
           int(penalty), int(median))
    return vec, cost


def warp(src, vec, step, fill=0):
    """src: uint8, bool or float32 CUDA tensor [N,1,H,W], [N,H,W] or [H,W]; vec: int32 [N,GH,GW,2] of ``block_match`` on the same device
    -> out(n, y, x) = src(n, y + dy, x + dx) with (dx, dy) the vector of the pixel's cell, ``fill`` where the source leaves the frame; the
    shape and dtype of ``src`` (bool goes through bytes).  An exact gather: float32 keeps its bits.  Enqueued only."""
    g.need_cuda(src, "src", "flow")
    g.need_cuda(vec, "vec", "flow")
    g.check_int("step", step, 1, FLOW_MAX_STEP, "flow")
    src, n, h, w = g.planes(src, "src", (torch.uint8, torch.bool, torch.float32), FLOW_MAX_SIDE)
    gh, gw = grid_shape(h, w, step)
    if vec.dtype != torch.int32 or tuple(vec.shape) != (n, gh, gw, 2) or vec.device != src.device:
        raise ValueError("vec must be an int32 [%d,%d,%d,2] tensor on the device of src, got %s %s" % (n, gh, gw, vec.dtype, tuple(vec.shape)))
    as_bool = src.dtype == torch.bool
    fill = float(fill)
    if src.dtype != torch.float32 and not (fill == int(fill) and 0 <= fill <= (1 if as_bool else 255)):
        raise ValueError("fill %r is no %s value" % (fill, "bool" if as_bool else "byte"))
    x = src.to(torch.uint8) if as_bool else src
    out = torch.empty_like(x)
    v = vec.contiguous()
    g.call("flow_warp", x.device, g.ptr(x), 1 if x.dtype == torch.float32 else 0, g.ptr(v), g.ptr(out), n, h, w, int(step), fill)
    return out.to(torch.bool) if as_bool else out


class MotionCompensator(object):
    """The motion field from the previous frame of a sequence to the current one, kept on the device.

    ``update(frames_u8)`` takes the decoded uint8 BGR frame(s) [N,H,W,3] or [H,W,3] in sequence order and computes the field of each: frame n
    of a batch is matched against frame n - 1, frame 0 against the frame stored by the call before; with no stored frame (the first call,
    or after ``reset``) the field of frame 0 is zero.  It then stores the last frame.  ``warp(x, fill=0)`` applies the field of the batch's
    FIRST frame to ``x`` (``flow.warp``); before any ``update`` it returns ``x`` unchanged.  ``vec`` / ``cost`` hold the fields [N,GH,GW,2]
    and costs [N,GH,GW] of the last update.  Enqueues only; nothing is read back.

    The defaults are starting values, NOT tuned on DAVIS."""

    def __init__(self, search=24, block=16, step=4, penalty=4, median=1):
        check_flow(search, block, step, penalty, median)
        self.search, self.block, self.step, self.penalty, self.median = int(search), int(block), int(step), int(penalty), int(median)
        self.vec = self.cost = None
        self._last = None
        self._ws = None

    def reset(self):
        """forget the stored frame and the field: the next ``update`` starts a sequence"""
        self._last = None
        self.vec = self.cost = None

    def update(self, frames_u8):
        cur = _frames(frames_u8, "frames_u8")
        if self._last is not None and (tuple(self._last.shape[1:]) != tuple(cur.shape[1:]) or self._last.device != cur.device):
            raise ValueError("frames of %s follow a frame of %s: call reset() between sequences" % (tuple(cur.shape[1:]), tuple(self._last.shape[1:])))
        n, h, w = (int(v) for v in cur.shape[:3])
        first = self._last is None
        # (with no stored frame, frame 0 is matched against itself: cost 0 at d = 0, the first candidate of the order -- a zero field)
        prev = torch.cat([cur[:1] if first else self._last, cur[:-1]]) if n > 1 else (cur if first else self._last)
        self._ws = workspace(n, h, w, self.block, self.step, self.search, self.median, cur.device, self._ws)
        self.vec, self.cost = block_match(prev, cur, self.search, self.block, self.step, self.penalty, self.median, ws=self._ws)
        self._last = cur[n - 1:].clone()
        return self.vec

    def warp(self, x, fill=0):
        if self.vec is None:
            return x
        if not torch.is_tensor(x) or x.dim() not in (2, 3, 4) or (x.dim() != 2 and x.shape[0] != 1):
            raise ValueError("MotionCompensator.warp takes one map ([1,1,H,W], [1,H,W] or [H,W]): the field of the batch's first frame")
        return warp(x, self.vec[:1], self.step, fill)
