"""Appearance matching to the annotated first frame (PML / VideoMatch / FEELVOS style), on the device: every pixel's trunk feature is
quantised to int8 and compared with the features of the first frame -- and optionally of the previous frame -- by a labelled
nearest-neighbour search on the integer matrix pipe (``osvos_match_quantize`` / ``osvos_match_cell_labels`` / ``osvos_match_nearest``,
csrc/match.hip; the rule: include/osvos_hip.h).

    quantise: q = clamp(rint(f * 127 / max|f|), -127, 127) per pixel, rinv = 1 / sqrt(sum q^2)
    labels:   a feature cell is object when 3/4 of its pixels are, background when at most 1/4 are, void (in neither bank) otherwise
    nearest:  per query pixel and class, the largest cosine dot(Q_a, R_b) * rinv_r[b] * rinv_q[a] over the bank's rows of that class
    map:      cosine to the nearest foreground feature minus cosine to the nearest background feature, on the feature grid
    topk:     in place of the nearest row, the mean cosine to the k best rows of the class (``osvos_match_topk``, csrc/match_ext.hip)
    local:    nearest over the reference cells within ``radius`` cells of the query cell on the same grid (``osvos_match_local``); its map
              counts a class the window does not hold as cosine -1

The network's logits are the only evidence every other stage has; when the network fires on a distractor that merely looks like the object
to its classifier, the map is a second opinion from the features themselves.  ``AppearanceMatcher`` adds ``gain * map`` to the fused logits
with ``tta.fuse_views`` (bilinear, on the device).  Integer dot products: the result is exact and repeats bit for bit.

The default parameters are STARTING VALUES, NOT TUNED ON DAVIS (no dataset was at hand when this was written), and no accuracy claim is
made for them: tune them on a validation split before quoting a score.
"""
import sys

import torch

from . import _glue as g
from . import tta
from ._lib import MATCH_MAX_C, MATCH_MAX_K, MATCH_MAX_P, MATCH_MAX_RADIUS, lib
from .autograd import FEATURE_LAYERS

_STRIDE = {3: 2, 6: 4, 9: 8, 12: 16}      # conv2_2, conv3_3, conv4_3, conv5_3: 2^stage under ceil-mode pooling


def stride_of(layer):
    """pixels per feature cell of trunk tensor ``layer`` (3, 6, 9 or 12)"""
    g.check_int("layer", layer, min(FEATURE_LAYERS), max(FEATURE_LAYERS), "match")
    if int(layer) not in FEATURE_LAYERS:
        raise ValueError("match: layer %r is not one of %s (conv2_2, conv3_3, conv4_3, conv5_3)" % (layer, FEATURE_LAYERS))
    return _STRIDE[int(layer)]


def check_match(layer, gain):
    """ValueError unless ``layer`` is one of the four feature layers and ``gain`` a finite number >= 0 (0 = off; host only)"""
    stride_of(layer)
    g.check_number("gain", gain, 0, None, "match")


def _channels_ok(c):
    return 64 <= c <= MATCH_MAX_C and c % 64 == 0


def quantize(feat):
    """feat: float32 or bfloat16 CUDA tensor [..., C] (C a multiple of 64, 64..1024; e.g. the [N,h,w,C] view of ``OSVOS.forward_features``)
    -> (q int8 [..., C], rinv float32 [...]).  Enqueued only."""
    g.need_cuda(feat, "feat", "match")
    if feat.dtype not in (torch.float32, torch.bfloat16) or feat.dim() < 2:
        raise ValueError("feat must be a float32 or bfloat16 [..., C] tensor, got %s %s" % (feat.dtype, tuple(feat.shape)))
    c = int(feat.shape[-1])
    if not _channels_ok(c) or feat.numel() == 0:
        raise ValueError("feat of %s: C must be a multiple of 64 in 64..%d and no dimension empty" % (tuple(feat.shape), MATCH_MAX_C))
    f = feat.contiguous()
    p = f.numel() // c
    q = torch.empty(f.shape, device=f.device, dtype=torch.int8)
    rinv = torch.empty(f.shape[:-1], device=f.device, dtype=torch.float32)
    g.call("match_quantize", f.device, g.ptr(f), 1 if f.dtype == torch.bfloat16 else 0, g.ptr(q), g.ptr(rinv), p, c)
    return q, rinv


def cell_labels(mask, stride):
    """mask: uint8 or bool CUDA tensor [N,H,W], [N,1,H,W] or [H,W], nonzero = object -> uint8 [N,h,w] on the ceil(H / stride) x ceil(W / stride)
    grid: 1 object, 0 background, 255 void.  Enqueued only."""
    g.need_cuda(mask, "mask", "match")
    m, n, H, W = g.planes(mask, "mask", (torch.uint8, torch.bool))
    if m.numel() == 0:
        raise ValueError("mask of %s: no dimension may be empty" % (tuple(mask.shape),))
    g.check_int("stride", stride, 1, 64, "match")
    if stride & (stride - 1):
        raise ValueError("match: stride %r (a power of two, 1..64)" % (stride,))
    if m.dtype == torch.bool:
        m = m.to(torch.uint8)
    h, w = g.grid_shape(H, W, stride)
    label = torch.empty((n, h, w), device=m.device, dtype=torch.uint8)
    g.call("match_cell_labels", m.device, g.ptr(m), g.ptr(label), n, H, W, h, w, int(stride))
    return label


def _operands(q, rinv_q, r, rinv_r, label_r):
    """the five tensors of a search, checked -> (the contiguous tensors, N, NR, Pq, Pr, C)"""
    for t, what in ((q, "q"), (rinv_q, "rinv_q"), (r, "r"), (rinv_r, "rinv_r"), (label_r, "label_r")):
        g.need_cuda(t, what, "match")
    if q.dtype != torch.int8 or r.dtype != torch.int8 or q.dim() != 3 or r.dim() != 3 or q.shape[2] != r.shape[2]:
        raise ValueError("q and r must be int8 [N,Pq,C] and [NR,Pr,C] tensors with the same C, got %s %s and %s %s" % (q.dtype, tuple(q.shape), r.dtype, tuple(r.shape)))
    n, pq, c = (int(v) for v in q.shape)
    nr, pr = int(r.shape[0]), int(r.shape[1])
    if not _channels_ok(c) or nr not in (1, n) or not (1 <= pq <= MATCH_MAX_P and 1 <= pr <= MATCH_MAX_P) or n < 1:
        raise ValueError("match: N %d NR %d Pq %d Pr %d C %d: NR is N or 1, rows 1..%d, C a multiple of 64 in 64..%d" % (n, nr, pq, pr, c, MATCH_MAX_P, MATCH_MAX_C))
    if rinv_q.dtype != torch.float32 or tuple(rinv_q.shape) != (n, pq) or rinv_r.dtype != torch.float32 or tuple(rinv_r.shape) != (nr, pr):
        raise ValueError("rinv_q and rinv_r must be float32 [%d,%d] and [%d,%d] tensors" % (n, pq, nr, pr))
    if label_r.dtype != torch.uint8 or tuple(label_r.shape) != (nr, pr):
        raise ValueError("label_r must be a uint8 [%d,%d] tensor, got %s %s" % (nr, pr, label_r.dtype, tuple(label_r.shape)))
    if any(t.device != q.device for t in (rinv_q, r, rinv_r, label_r)):
        raise ValueError("match: the five tensors must be on one device")
    q, rinv_q, r, rinv_r, label_r = (t.contiguous() for t in (q, rinv_q, r, rinv_r, label_r))
    return (q, rinv_q, r, rinv_r, label_r), n, nr, pq, pr, c


def nearest_workspace(n, pq, pr, c, device, ws=None):
    """a uint8 CUDA tensor of at least osvos_match_ws_bytes: ``ws`` when it is large enough and on ``device``, else a new one"""
    return g.workspace(lib().osvos_match_ws_bytes(n, pq, pr, c), device, ws, "N %d Pq %d Pr %d C %d" % (n, pq, pr, c), "match")


def nearest(q, rinv_q, r, rinv_r, label_r, ws=None, with_idx=False):
    """q int8 [N,Pq,C] with rinv_q float32 [N,Pq]; r int8 [NR,Pr,C] with rinv_r float32 and label_r uint8 [NR,Pr], NR = N or 1 (one bank for
    every frame) -> sim float32 [N,2,Pq]: per query row the cosine to the nearest reference row labelled 1 (row 0 of the class axis) and to
    the nearest labelled 0 (row 1); -2 for a class the bank does not hold.  ``with_idx``: also idx int32 [N,2,Pq], the smallest reference
    row that attains it (-1 for an empty class).  Enqueued only."""
    (q, rinv_q, r, rinv_r, label_r), n, nr, pq, pr, c = _operands(q, rinv_q, r, rinv_r, label_r)
    sim = torch.empty((n, 2, pq), device=q.device, dtype=torch.float32)
    idx = torch.empty((n, 2, pq), device=q.device, dtype=torch.int32) if with_idx else None
    ws = nearest_workspace(n, pq, pr, c, q.device, ws)
    g.call("match_nearest", q.device, g.ptr(q), g.ptr(rinv_q), g.ptr(r), g.ptr(rinv_r), g.ptr(label_r), g.ptr(sim), g.ptr(idx), g.ptr(ws), n, nr, pq,
           pr, c)
    return (sim, idx) if with_idx else sim


def topk_workspace(n, pq, pr, c, k, device, ws=None):
    """a uint8 CUDA tensor of at least osvos_match_topk_ws_bytes: ``ws`` when it is large enough and on ``device``, else a new one"""
    g.check_int("k", k, 1, MATCH_MAX_K, "match")
    return g.workspace(lib().osvos_match_topk_ws_bytes(n, pq, pr, c, int(k)), device, ws, "N %d Pq %d Pr %d C %d K %d" % (n, pq, pr, c, k), "match")


def topk(q, rinv_q, r, rinv_r, label_r, k, ws=None):
    """the operands of ``nearest`` -> sim float32 [N,2,Pq]: per query row and class the mean cosine to the ``k`` (1..16) best reference rows
    of the class -- to all of them when the bank holds fewer, -2 when it holds none; summed from the best down and divided once
    (VideoMatch's averaging: one mislabelled bank row no longer decides).  ``k`` = 1 gives ``nearest``'s bits.  Enqueued only."""
    g.check_int("k", k, 1, MATCH_MAX_K, "match")
    (q, rinv_q, r, rinv_r, label_r), n, nr, pq, pr, c = _operands(q, rinv_q, r, rinv_r, label_r)
    sim = torch.empty((n, 2, pq), device=q.device, dtype=torch.float32)
    ws = topk_workspace(n, pq, pr, c, k, q.device, ws)
    g.call("match_topk", q.device, g.ptr(q), g.ptr(rinv_q), g.ptr(r), g.ptr(rinv_r), g.ptr(label_r), g.ptr(sim), g.ptr(ws), n, nr, pq, pr, c, int(k))
    return sim


def local(q, rinv_q, r, rinv_r, label_r, grid, radius, with_idx=False):
    """the operands of ``nearest`` with Pq = Pr = h w, both row-major on the ``grid`` = (h, w) -> sim float32 [N,2,P]: per query cell and
    class the cosine to the nearest reference cell of the class at most ``radius`` (0..15) rows and columns away; -2 when the window holds
    none.  ``with_idx``: also idx int32 [N,2,P], the smallest reference row that attains it (-1).  FEELVOS's local map.  Enqueued only."""
    g.check_int("radius", radius, 0, MATCH_MAX_RADIUS, "match")
    if not isinstance(grid, (tuple, list)) or len(grid) != 2:
        raise ValueError("match: grid must be (h, w), got %r" % (grid,))
    h, w = grid
    g.check_int("grid h", h, 1, MATCH_MAX_P, "match")
    g.check_int("grid w", w, 1, MATCH_MAX_P, "match")
    (q, rinv_q, r, rinv_r, label_r), n, nr, pq, pr, c = _operands(q, rinv_q, r, rinv_r, label_r)
    if pq != h * w or pr != h * w:
        raise ValueError("match: Pq %d and Pr %d must both be the grid's %d x %d = %d cells" % (pq, pr, h, w, h * w))
    sim = torch.empty((n, 2, pq), device=q.device, dtype=torch.float32)
    idx = torch.empty((n, 2, pq), device=q.device, dtype=torch.int32) if with_idx else None
    g.call("match_local", q.device, g.ptr(q), g.ptr(rinv_q), g.ptr(r), g.ptr(rinv_r), g.ptr(label_r), g.ptr(sim), g.ptr(idx), n, nr, int(h), int(w), c,
           int(radius))
    return (sim, idx) if with_idx else sim


def local_map(sim):
    """sim [N,2,P] of ``local`` -> max(sim_fg, -1) - max(sim_bg, -1), float32 [N,P]: a class the window does not hold counts as the smallest
    possible cosine, so "no object was near here a frame ago" is evidence against the object"""
    return torch.clamp_min(sim[:, 0], -1.0) - torch.clamp_min(sim[:, 1], -1.0)


def check_match_options(topk, local_radius, local_gain):
    """ValueError unless ``topk`` is in 1..16, ``local_radius`` in 0..15 and ``local_gain`` a finite number >= 0 (0 = off; host only)"""
    g.check_int("topk", topk, 1, MATCH_MAX_K, "match")
    g.check_int("local_radius", local_radius, 0, MATCH_MAX_RADIUS, "match")
    g.check_number("local_gain", local_gain, 0, None, "match")


class AppearanceMatcher(object):
    """A second opinion on the fused logits from the trunk features themselves, on the device.

    ``matcher.set_reference(x0, mask0)`` runs the annotated first frame ``x0`` [1,3,H,W] through ``net`` and keeps the int8 features of
    trunk tensor ``layer`` with the cell labels of ``mask0`` (uint8 or bool [H,W], [1,H,W] or [1,1,H,W]) as the first-frame bank.  ONE
    read-back checks that the bank holds both classes; if it does not, the matcher is inert -- it says so once and returns plain forwards.

    ``matcher(x, prev_mask=None)`` runs ``net.forward_features(x)``, quantises the features, searches the bank, and returns the five logit
    maps of the forward with the last one replaced by ``tta.fuse_views([fused, map], .., weights=[1, gain])``, map = cosine to the nearest
    foreground feature minus cosine to the nearest background feature.  With ``previous=True`` the features of the previous call and
    ``prev_mask`` (that frame's final mask [N,H,W] or [N,1,H,W]) form a second bank, and each class takes the larger of its two cosines.
    ``gain == 0`` is ``net.forward`` under ``torch.no_grad()`` and nothing else.  The banks and workspaces stay on the device.

    ``topk`` > 1 searches both banks with ``topk`` in place of ``nearest``: a class's score is the mean cosine to its ``topk`` best rows.
    ``local_gain`` > 0 adds a THIRD view to the same ``fuse_views`` call, weights ``[1, gain, local_gain]``: ``local_map`` of the search of
    the previous call's features under ``prev_mask`` within ``local_radius`` cells of each pixel (``local``).  It does not depend on
    ``previous``; on the first matched frame, or without ``prev_mask``, there is no local view.  ``topk=1, local_gain=0`` is the matcher
    without these options: the same calls, the same bytes.

    The defaults are starting values, NOT tuned on DAVIS."""

    def __init__(self, net, layer=9, gain=4.0, previous=False, topk=1, local_radius=0, local_gain=0.0):
        check_match(layer, gain)
        check_match_options(topk, local_radius, local_gain)
        self.net, self.layer, self.gain, self.previous = net, int(layer), float(gain), bool(previous)
        self.topk, self.local_radius, self.local_gain = int(topk), int(local_radius), float(local_gain)
        self.stride = stride_of(layer)
        self.inert = False
        self._bank = None            # (r [1,P,C], rinv_r [1,P], label [1,P]) of the first frame
        self._last = None            # (q, rinv_q) of the previous call
        self._ws = self._ws_prev = None

    @property
    def has_reference(self):
        """True once set_reference has run (or when gain is 0 and there is nothing to build)"""
        return self.gain == 0 or self._bank is not None

    @property
    def needs_previous(self):
        """True when the next call wants this call's features and mask: the previous-frame bank, the local view, or both"""
        return self.previous or self.local_gain > 0

    def _search(self, q, rinv_q, r, rinv_r, label, which):
        """one bank: ``nearest``, or ``topk`` when topk > 1; ``which`` names the bank's workspace attribute"""
        n, p, c = (int(v) for v in q.shape)
        if self.topk > 1:
            ws = topk_workspace(n, p, p, c, self.topk, q.device, getattr(self, which))
            setattr(self, which, ws)
            return topk(q, rinv_q, r, rinv_r, label, self.topk, ws=ws)
        ws = nearest_workspace(n, p, p, c, q.device, getattr(self, which))
        setattr(self, which, ws)
        return nearest(q, rinv_q, r, rinv_r, label, ws=ws)

    def _features(self, x):
        outs, feat, _ = self.net.forward_features(x, self.layer)
        n, h, w, c = (int(v) for v in feat.shape)
        q, rinv = quantize(feat)
        return outs, q.view(n, h * w, c), rinv.view(n, h * w), (h, w)

    def set_reference(self, x0, mask0):
        if self.gain == 0:
            return self
        if x0.dim() != 4 or x0.shape[0] != 1:
            raise ValueError("set_reference takes ONE annotated frame [1,3,H,W], got %s" % (tuple(x0.shape),))
        _, r, rinv_r, (h, w) = self._features(x0)
        label = cell_labels(mask0, self.stride)
        if tuple(label.shape) != (1, h, w):
            raise ValueError("mask0 of %s does not belong to a frame of %s" % (tuple(mask0.shape), tuple(x0.shape)))
        label = label.view(1, h * w)
        n_fg, n_bg = (int(v) for v in torch.stack([(label == 1).sum(), (label == 0).sum()]).cpu().numpy())      # the one read-back
        self.inert = n_fg == 0 or n_bg == 0
        if self.inert:
            print("AppearanceMatcher: the first frame gives %d foreground and %d background cells at layer %d (stride %d): no matching, plain forwards"
                  % (n_fg, n_bg, self.layer, self.stride), file=sys.stderr)
        self._bank, self._last = (r, rinv_r, label), None
        return self

    def __call__(self, x, prev_mask=None):
        if self.gain == 0:
            with torch.no_grad():
                return self.net.forward(x)
        if self._bank is None:
            raise RuntimeError("AppearanceMatcher: set_reference(first frame, its mask) comes first")
        if self.inert:
            return self.net.forward_features(x, self.layer)[0]
        outs, q, rinv_q, (h, w) = self._features(x)
        n, p, c = (int(v) for v in q.shape)
        r, rinv_r, label = self._bank
        if int(r.shape[1]) != p:
            raise ValueError("AppearanceMatcher: the frame's %d x %d feature grid is not the first frame's" % (h, w))
        sim = self._search(q, rinv_q, r, rinv_r, label, "_ws")
        local_mp = None
        if self.needs_previous:
            if prev_mask is not None and self._last is not None and self._last[0].shape == q.shape:
                plabel = cell_labels(prev_mask, self.stride)
                if tuple(plabel.shape) != (n, h, w):
                    raise ValueError("prev_mask of %s does not belong to frames of %s" % (tuple(prev_mask.shape), tuple(x.shape)))
                if self.previous:
                    sim = torch.maximum(sim, self._search(q, rinv_q, self._last[0], self._last[1], plabel.view(n, p), "_ws_prev"))
                if self.local_gain > 0:
                    local_mp = local_map(local(q, rinv_q, self._last[0], self._last[1], plabel.view(n, p), (h, w), self.local_radius)).view(n, h, w)
            self._last = (q, rinv_q)
        views, weights = [outs[-1], (sim[:, 0] - sim[:, 1]).view(n, h, w)], [1.0, self.gain]
        if local_mp is not None:
            views, weights = views + [local_mp], weights + [self.local_gain]
        fused = tta.fuse_views(views, [False] * len(views), (int(x.shape[2]), int(x.shape[3])), weights=weights)
        return list(outs[:4]) + [fused]
