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
    memory:   a fixed-capacity bank behind the first frame's rows that collects, frame after frame, the rows the bank does not hold yet and the
              mask confirms (``osvos_match_bank_update``, csrc/match_bank.hip; ``MemoryBank``): the oldest rows are overwritten first, the first
              frame's never
    soft:     in place of one row per class, every row of the class votes with weight exp(beta (cosine - 1)) and the class's score is
              1 + ln(sum of its weights) / beta, between its largest cosine and that plus ln(rows) / beta (``osvos_match_soft``,
              csrc/match_soft.hip): the softmax read of STM, STCN and XMem over the labels; one mislabelled or drifted row is outvoted

The network's logits are the only evidence every other stage has; when the network fires on a distractor that merely looks like the object
to its classifier, the map is a second opinion from the features themselves.  ``AppearanceMatcher`` adds ``gain * map`` to the fused logits
with ``tta.fuse_views`` (bilinear, on the device).  Integer dot products: the result is exact and repeats bit for bit (the soft readout
repeats bit for bit too, and agrees with its restatement within the error of the hardware exponential and of a float32 sum).

The default parameters are STARTING VALUES, NOT TUNED ON DAVIS (no dataset was at hand when this was written), and no accuracy claim is
made for them: tune them on a validation split before quoting a score.
"""
import sys

import torch

from . import _glue as g
from . import tta
from ._lib import MATCH_MAX_BETA, MATCH_MAX_C, MATCH_MAX_K, MATCH_MAX_P, MATCH_MAX_RADIUS, MATCH_MIN_BETA, lib
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


def check_soft(beta, balance=False):
    """ValueError unless ``beta`` is 0 (off) or a finite number in 1/16..40 and ``balance`` a bool (host only)"""
    g.check_number("soft_beta", beta, 0, MATCH_MAX_BETA, "match")
    if 0 < beta < MATCH_MIN_BETA:
        raise ValueError("match: soft_beta %r (0 = off, or a finite number in %g..%g)" % (beta, MATCH_MIN_BETA, MATCH_MAX_BETA))
    if not isinstance(balance, bool):
        raise ValueError("match: soft_balance must be True or False, got %r" % (balance,))


def soft_workspace(n, pq, pr, c, device, ws=None):
    """a uint8 CUDA tensor of at least osvos_match_soft_ws_bytes: ``ws`` when it is large enough, 8-byte aligned and on ``device``, else a new one"""
    return g.workspace(lib().osvos_match_soft_ws_bytes(n, pq, pr, c), device, ws, "N %d Pq %d Pr %d C %d" % (n, pq, pr, c), "match", align=8)


def soft(q, rinv_q, r, rinv_r, label_r, beta, ws=None, with_best=False):
    """the operands of ``nearest`` and a temperature ``beta`` (1/16..40) -> lse float32 [N,2,Pq]: per query row and class
    1 + ln(sum over the class's rows of exp(beta (cosine - 1))) / beta -- the class's largest cosine when one row dominates, up to
    ln(rows) / beta more when many rows are as near; -2 for a class the bank does not hold.  beta (lse_fg - lse_bg) is the log-odds of the
    object under a softmax over every row of the bank (STM's read with the label as the value).  ``with_best``: also best float32 [N,2,Pq],
    ``nearest``'s sim bit for bit, from the same pass.  Enqueued only."""
    check_soft(beta)
    if not beta > 0:
        raise ValueError("match: soft takes a temperature in %g..%g, got %r" % (MATCH_MIN_BETA, MATCH_MAX_BETA, beta))
    (q, rinv_q, r, rinv_r, label_r), n, nr, pq, pr, c = _operands(q, rinv_q, r, rinv_r, label_r)
    lse = torch.empty((n, 2, pq), device=q.device, dtype=torch.float32)
    best = torch.empty((n, 2, pq), device=q.device, dtype=torch.float32) if with_best else None
    ws = soft_workspace(n, pq, pr, c, q.device, ws)
    g.call("match_soft", q.device, g.ptr(q), g.ptr(rinv_q), g.ptr(r), g.ptr(rinv_r), g.ptr(label_r), g.ptr(lse), g.ptr(best), g.ptr(ws), n, nr, pq, pr,
           c, float(beta))
    return (lse, best) if with_best else lse


def soft_rows(label_r):
    """label_r uint8 [NR,Pr] -> float32 [NR,2,1]: the rows of the foreground and of the background, counted on the device (no read-back)"""
    return torch.stack([(label_r == 1).sum(dim=1), (label_r == 0).sum(dim=1)], dim=1).to(torch.float32)[:, :, None]


def soft_union(a, b, beta):
    """lse [N,2,Pq] of two banks -> that of their union, logaddexp(beta a, beta b) / beta: the softmax over both banks' rows.  A class a
    bank does not hold (-2) counts as minus infinity; -2 when neither holds it"""
    inf = float("inf")
    x, y = (torch.where(t == -2.0, torch.full_like(t, -inf), t * beta) for t in (a, b))
    u = torch.logaddexp(x, y) / beta
    return torch.where((a == -2.0) & (b == -2.0), torch.full_like(u, -2.0), u)


def soft_balanced(lse, rows, beta):
    """lse [N,2,Pq] minus ln(rows) / beta per class (``rows`` of ``soft_rows``): the MEAN of the weights in place of their sum, so that a bank
    with ten times more background rows carries no prior.  An empty class stays -2"""
    return torch.where(rows > 0, lse - torch.log(torch.clamp_min(rows, 1.0)) / beta, lse)


def check_match_options(topk, local_radius, local_gain):
    """ValueError unless ``topk`` is in 1..16, ``local_radius`` in 0..15 and ``local_gain`` a finite number >= 0 (0 = off; host only)"""
    g.check_int("topk", topk, 1, MATCH_MAX_K, "match")
    g.check_int("local_radius", local_radius, 0, MATCH_MAX_RADIUS, "match")
    g.check_number("local_gain", local_gain, 0, None, "match")


def check_memory(memory, memory_tau=0.9, memory_new=512, memory_margin=0.0):
    """ValueError unless ``memory`` is an integer in 0..2^20 - 1 (rows of the ring; 0 = off), ``memory_new`` an integer >= 0 and ``memory_tau`` and
    ``memory_margin`` finite numbers (host only)"""
    g.check_int("memory", memory, 0, MATCH_MAX_P - 1, "match")
    g.check_number("memory_tau", memory_tau, -float(1 << 30), float(1 << 30), "match")
    g.check_int("memory_new", memory_new, 0, 1 << 30, "match")
    g.check_number("memory_margin", memory_margin, -float(1 << 30), float(1 << 30), "match")


def bank_workspace(n, p, device, ws=None):
    """a uint8 CUDA tensor of at least osvos_match_bank_ws_bytes: ``ws`` when it is large enough, 8-byte aligned and on ``device``, else a new one"""
    return g.workspace(lib().osvos_match_bank_ws_bytes(n, p), device, ws, "N %d P %d" % (n, p), "match", align=8)


def bank_update(q, rinv_q, label_q, sim, r, rinv_r, label_r, state, max_new, tau, margin, protected, ws=None):
    """one ``osvos_match_bank_update``: the rows of N frames -- q int8 [N,P,C], rinv_q float32 [N,P], label_q uint8 [N,P] (``cell_labels`` of the
    frame's mask) and sim float32 [N,2,P], the search of these rows against the banks -- are added IN PLACE to the N banks r int8 [N,cap,C],
    rinv_r float32 [N,cap], label_r uint8 [N,cap] with state int32 [N,4], whose rows below ``protected`` are never written (the rule:
    include/osvos_hip.h).  Enqueued only; -> the workspace it used."""
    for t, what in ((q, "q"), (rinv_q, "rinv_q"), (label_q, "label_q"), (sim, "sim"), (r, "r"), (rinv_r, "rinv_r"), (label_r, "label_r"), (state, "state")):
        g.need_cuda(t, what, "match")
    check_memory(0, tau, max_new, margin)
    if q.dtype != torch.int8 or r.dtype != torch.int8 or q.dim() != 3 or r.dim() != 3 or q.shape[2] != r.shape[2] or q.shape[0] != r.shape[0]:
        raise ValueError("q and r must be int8 [N,P,C] and [N,cap,C] tensors with the same N and C, got %s %s and %s %s"
                         % (q.dtype, tuple(q.shape), r.dtype, tuple(r.shape)))
    n, p, c = (int(v) for v in q.shape)
    cap = int(r.shape[1])
    if not _channels_ok(c) or n < 1 or not (1 <= p <= MATCH_MAX_P and 1 <= cap <= MATCH_MAX_P):
        raise ValueError("match: N %d P %d cap %d C %d: rows 1..%d, C a multiple of 64 in 64..%d" % (n, p, cap, c, MATCH_MAX_P, MATCH_MAX_C))
    g.check_int("protected", protected, 0, cap, "match")
    want = ((rinv_q, "rinv_q", torch.float32, (n, p)), (label_q, "label_q", torch.uint8, (n, p)), (sim, "sim", torch.float32, (n, 2, p)),
            (rinv_r, "rinv_r", torch.float32, (n, cap)), (label_r, "label_r", torch.uint8, (n, cap)), (state, "state", torch.int32, (n, 4)))
    for t, what, dtype, shape in want:
        if t.dtype != dtype or tuple(t.shape) != shape or t.device != q.device:
            raise ValueError("%s must be a %s %s tensor on the device of q, got %s %s" % (what, str(dtype).replace("torch.", ""), list(shape), t.dtype,
                                                                                          tuple(t.shape)))
    for t, what in ((r, "r"), (rinv_r, "rinv_r"), (label_r, "label_r"), (state, "state")):      # written in place: no copy may stand in for them
        if not t.is_contiguous():
            raise ValueError("match: %s is written in place and must be contiguous" % what)
    q, rinv_q, label_q, sim = (t.contiguous() for t in (q, rinv_q, label_q, sim))
    ws = bank_workspace(n, p, q.device, ws)
    g.call("match_bank_update", q.device, g.ptr(q), g.ptr(rinv_q), g.ptr(label_q), g.ptr(sim), g.ptr(r), g.ptr(rinv_r), g.ptr(label_r), g.ptr(state),
           g.ptr(ws), n, p, c, cap, int(protected), int(max_new), float(tau), float(margin))
    return ws


class MemoryBank(object):
    """The first frame's rows and, behind them, a ring of ``capacity_rows`` rows that ``update`` fills over the sequence, all on the device.

    ``seed(r0, rinv0, label0)`` -- int8 [1,P0,C], float32 [1,P0], uint8 [1,P0] -- allocates [1, P0 + capacity_rows, C]: the first frame's rows
    with their labels as they are (protected: no update writes them), the ring void (label 255, everything else zero), ``state`` zero.
    ``update(q, rinv_q, label_q, sim)`` admits at most ``max_new`` rows of a frame that was searched against this bank: those with a 0 / 1 label
    whose own-class cosine is below ``tau`` (the bank does not hold them yet) and at least ``margin`` above the other class's (the bank does not
    contradict the label), evenly subsampled, over the oldest ring rows.  One library call, no read-back.
    ``rows`` is the host's bound on the rows written so far, protected + min(ring, calls * min(max_new, ring)); ``operands()`` the three bank
    tensors narrowed to it.  Rows past what was really written are void, so the bound costs time when it is loose and never a bit.

    The defaults are starting values, NOT tuned on DAVIS."""

    def __init__(self, capacity_rows, tau=0.9, max_new=512, margin=0.0):
        check_memory(capacity_rows, tau, max_new, margin)
        if capacity_rows < 1:
            raise ValueError("match: MemoryBank of %d rows (1..%d)" % (capacity_rows, MATCH_MAX_P - 1))
        self.capacity_rows, self.tau, self.max_new, self.margin = int(capacity_rows), float(tau), int(max_new), float(margin)
        self.protected = self.host_calls = 0
        self.r = self.rinv_r = self.label_r = self.state = self._ws = None

    @property
    def ring(self):
        return self.capacity_rows

    @property
    def rows(self):
        return self.protected + min(self.ring, self.host_calls * min(self.max_new, self.ring))

    def seed(self, r0, rinv0, label0):
        for t, what in ((r0, "r0"), (rinv0, "rinv0"), (label0, "label0")):
            g.need_cuda(t, what, "match")
        if r0.dtype != torch.int8 or r0.dim() != 3 or r0.shape[0] != 1 or not _channels_ok(int(r0.shape[2])):
            raise ValueError("r0 must be an int8 [1,P0,C] tensor, C a multiple of 64 in 64..%d, got %s %s" % (MATCH_MAX_C, r0.dtype, tuple(r0.shape)))
        p0, c = int(r0.shape[1]), int(r0.shape[2])
        if not 1 <= p0 <= MATCH_MAX_P - self.capacity_rows:
            raise ValueError("match: %d first-frame rows and %d memory rows (together 2..%d)" % (p0, self.capacity_rows, MATCH_MAX_P))
        if rinv0.dtype != torch.float32 or tuple(rinv0.shape) != (1, p0) or label0.dtype != torch.uint8 or tuple(label0.shape) != (1, p0):
            raise ValueError("rinv0 and label0 must be float32 and uint8 [1,%d] tensors" % p0)
        cap, dev = p0 + self.capacity_rows, r0.device
        self.r = torch.zeros((1, cap, c), device=dev, dtype=torch.int8)
        self.rinv_r = torch.zeros((1, cap), device=dev, dtype=torch.float32)
        self.label_r = torch.full((1, cap), 255, device=dev, dtype=torch.uint8)
        self.state = torch.zeros((1, 4), device=dev, dtype=torch.int32)
        self.r[:, :p0].copy_(r0)
        self.rinv_r[:, :p0].copy_(rinv0)
        self.label_r[:, :p0].copy_(label0)
        self.protected, self.host_calls = p0, 0
        return self

    def update(self, q, rinv_q, label_q, sim):
        if self.r is None:
            raise RuntimeError("MemoryBank: seed(first frame's rows) comes first")
        self._ws = bank_update(q, rinv_q, label_q, sim, self.r, self.rinv_r, self.label_r, self.state, self.max_new, self.tau, self.margin,
                               self.protected, ws=self._ws)
        self.host_calls += 1

    def operands(self):
        rows = self.rows
        return self.r[:, :rows], self.rinv_r[:, :rows], self.label_r[:, :rows]


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

    ``memory`` > 0 searches a ``MemoryBank(memory, memory_tau, memory_new, memory_margin)`` in place of the first-frame bank: the first frame's
    rows and a ring of ``memory`` rows behind them.  When ``prev_mask`` arrives, the previous call's rows, that call's search result against
    the bank (taken before the previous-frame bank was combined in) and the cell labels of ``prev_mask`` update the bank, on the device,
    before the new frame is searched; frames come one at a time then (N = 1).  ``memory=0`` is the matcher without it: the same calls, the
    same bytes.

    ``soft_beta`` > 0 reads every bank with ``soft`` in place of ``nearest``: the map is lse_fg - lse_bg, 1 / beta times the log-odds of the
    object under a softmax over all rows of the bank.  With ``previous=True`` the two banks combine as the softmax over their union
    (``soft_union``).  ``soft_balance=True`` subtracts ln(rows of the class) / beta per class -- the rows actually searched, both banks',
    counted on the device -- so that the larger class carries no prior.  With ``memory`` > 0 the search also returns ``nearest``'s sim from
    the same pass and THAT is what ``MemoryBank.update`` receives: the bank evolves exactly as without the soft readout.  Not with
    ``topk`` > 1 (a softmax over the top k rows is not built); the local view is unchanged.  ``soft_beta=0`` is the matcher without it: the
    same calls, the same bytes.  Beta 10 is a starting value.

    The defaults are starting values, NOT tuned on DAVIS."""

    def __init__(self, net, layer=9, gain=4.0, previous=False, topk=1, local_radius=0, local_gain=0.0, memory=0, memory_tau=0.9, memory_new=512,
                 memory_margin=0.0, soft_beta=0.0, soft_balance=False):
        check_match(layer, gain)
        check_match_options(topk, local_radius, local_gain)
        check_memory(memory, memory_tau, memory_new, memory_margin)
        check_soft(soft_beta, soft_balance)
        if soft_beta > 0 and topk > 1:
            raise ValueError("match: soft_beta %g with topk %d: the soft readout sums over every row of a class; a softmax over the top k is not built"
                             % (soft_beta, topk))
        self.soft_beta, self.soft_balance = float(soft_beta), bool(soft_balance)
        self.memory, self.memory_tau, self.memory_new, self.memory_margin = int(memory), float(memory_tau), int(memory_new), float(memory_margin)
        self._memory = None          # the MemoryBank (memory > 0), seeded by set_reference
        self.net, self.layer, self.gain, self.previous = net, int(layer), float(gain), bool(previous)
        self.topk, self.local_radius, self.local_gain = int(topk), int(local_radius), float(local_gain)
        self.stride = stride_of(layer)
        self.inert = False
        self._bank = None            # (r [1,P,C], rinv_r [1,P], label [1,P]) of the first frame
        self._last = None            # (q, rinv_q) of the previous call; with memory also its sim against the memory bank
        self._ws = self._ws_prev = None

    @property
    def has_reference(self):
        """True once set_reference has run (or when gain is 0 and there is nothing to build)"""
        return self.gain == 0 or self._bank is not None

    @property
    def needs_previous(self):
        """True when the next call wants this call's features and mask: the previous-frame bank, the local view, the memory bank, or several"""
        return self.previous or self.local_gain > 0 or self.memory > 0

    def _search(self, q, rinv_q, r, rinv_r, label, which):
        """one bank: ``nearest``, or ``topk`` when topk > 1; ``which`` names the bank's workspace attribute"""
        n, p, c = (int(v) for v in q.shape)
        pr = int(r.shape[1])
        if self.topk > 1:
            ws = topk_workspace(n, p, pr, c, self.topk, q.device, getattr(self, which))
            setattr(self, which, ws)
            return topk(q, rinv_q, r, rinv_r, label, self.topk, ws=ws)
        ws = nearest_workspace(n, p, pr, c, q.device, getattr(self, which))
        setattr(self, which, ws)
        return nearest(q, rinv_q, r, rinv_r, label, ws=ws)

    def _search_soft(self, q, rinv_q, r, rinv_r, label, which, with_best=False):
        """one bank under the soft readout -> (lse, ``nearest``'s sim or None, the bank's rows per class)"""
        n, p, c = (int(v) for v in q.shape)
        ws = soft_workspace(n, p, int(r.shape[1]), c, q.device, getattr(self, which))
        setattr(self, which, ws)
        out = soft(q, rinv_q, r, rinv_r, label, self.soft_beta, ws=ws, with_best=with_best)
        lse, best = out if with_best else (out, None)
        return lse, best, soft_rows(label) if self.soft_balance else None

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
        self._memory = MemoryBank(self.memory, self.memory_tau, self.memory_new, self.memory_margin).seed(r, rinv_r, label) if self.memory > 0 else None
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
        if self._memory is not None and n != 1:
            raise ValueError("AppearanceMatcher: with memory the frames come one at a time, got %d" % n)

        def prev_labels():
            """the cell labels of prev_mask, or None without a previous frame of this shape: computed once for the memory bank, the
            previous-frame bank and the local view"""
            if prev_mask is None or self._last is None or self._last[0].shape != q.shape:
                return None
            plabel = cell_labels(prev_mask, self.stride)
            if tuple(plabel.shape) != (n, h, w):
                raise ValueError("prev_mask of %s does not belong to frames of %s" % (tuple(prev_mask.shape), tuple(x.shape)))
            return plabel

        plabel = None
        if self._memory is not None:                                         # the bank takes the previous frame in BEFORE this one is searched
            plabel = prev_labels()
            if plabel is not None:
                self._memory.update(self._last[0], self._last[1], plabel.view(n, p), self._last[2])
            r, rinv_r, label = self._memory.operands()
        soft_on, rows = self.soft_beta > 0, None
        if soft_on:                                                          # (first: nearest's sim from the same pass, for the memory bank)
            sim, first, rows = self._search_soft(q, rinv_q, r, rinv_r, label, "_ws", with_best=self._memory is not None)
        else:
            sim = first = self._search(q, rinv_q, r, rinv_r, label, "_ws")
        local_mp = None
        if self.needs_previous:
            if self._memory is None:
                plabel = prev_labels()
            if plabel is not None:
                if self.previous and soft_on:                                # the softmax over the union of the two banks
                    other, _, prows = self._search_soft(q, rinv_q, self._last[0], self._last[1], plabel.view(n, p), "_ws_prev")
                    sim, rows = soft_union(sim, other, self.soft_beta), rows + prows if self.soft_balance else None
                elif self.previous:
                    sim = torch.maximum(sim, self._search(q, rinv_q, self._last[0], self._last[1], plabel.view(n, p), "_ws_prev"))
                if self.local_gain > 0:
                    local_mp = local_map(local(q, rinv_q, self._last[0], self._last[1], plabel.view(n, p), (h, w), self.local_radius)).view(n, h, w)
            self._last = (q, rinv_q, first) if self._memory is not None else (q, rinv_q)
        if rows is not None:
            sim = soft_balanced(sim, rows, self.soft_beta)
        views, weights = [outs[-1], (sim[:, 0] - sim[:, 1]).view(n, h, w)], [1.0, self.gain]
        if local_mp is not None:
            views, weights = views + [local_mp], weights + [self.local_gain]
        fused = tta.fuse_views(views, [False] * len(views), (int(x.shape[2]), int(x.shape[3])), weights=weights)
        return list(outs[:4]) + [fused]
