"""Result writer and evaluator for the per-sequence test loop (reference train_online.py:181-189).

The reference turns the fused logit map into a probability (``1 / (1 + exp(-x))``), hands it to ``scipy.misc.imsave``
(scipy <= 1.1: min-max byte scaling, PIL mode 'L') and leaves the DAVIS evaluation to an external toolkit.  Here the
sigmoid + byte scaling run on the device (``osvos_mask_to_bytes``: one byte per pixel crosses PCIe instead of four),
the PNG is written by a small zlib encoder (no PIL / scipy dependency), and the two DAVIS measures -- region similarity J
(Jaccard index of the thresholded mask) and contour accuracy F (boundary precision / recall within a disk of 0.8 % of the
image diagonal) -- with their mean / recall / decay statistics and the headline J&F are computed from device-side integer
counts (``osvos_mask_iou_counts``, ``osvos_mask_jf_counts``); ``SequenceEvaluator`` keeps the counts of a whole sequence on
the device and reads them back once.

Multi-object sequences (DAVIS 2017: one fine-tuned network per object) end in the second half of this file: ``merge_objects`` turns the K
logit stacks into one uint8 label map per frame on the device (``osvos_merge_objects``), ``save_label_maps`` writes them as indexed PNGs with
the DAVIS palette, and ``MultiObjectEvaluator`` keeps J and F counts per frame AND object on the device (``osvos_labels_jf_counts``).

Mask clean-up sits between the logits and all of these: ``components`` labels the connected components of the thresholded mask on the device
(``osvos_mask_components``), ``filter_components`` drops components by area, rank or distance from a seed mask (``osvos_components_select``),
and ``ComponentTracker`` chains the seed test from frame to frame without reading anything back.
"""
import ctypes as C
import math
import struct
import zlib

import numpy as np
import torch

from . import _glue as g
from ._lib import BOUNDARY_MAX_RADIUS, MAX_OBJECTS, SQDIST_MAX_SIDE, lib


def _threshold_logit(threshold):
    if not 0.0 < threshold < 1.0:
        raise ValueError("threshold must be a probability in (0, 1)")
    return float(np.log(threshold / (1.0 - threshold)))


def mask_bytes(logits):
    """logits: float32 CUDA tensor [N,1,H,W] or [N,H,W] -> uint8 CUDA tensor [N,H,W] (imsave's byte image per frame)."""
    g.need_cuda(logits, "logits", "results")
    x = logits.detach().float().contiguous()
    n = x.shape[0]
    out = torch.empty((n,) + tuple(x.shape[-2:]), device=x.device, dtype=torch.uint8)
    scratch = torch.empty(2 * n, device=x.device, dtype=torch.int32)
    g.call("mask_to_bytes", x.device, g.ptr(x), g.ptr(out), g.ptr(scratch), x.numel() // n, n)
    return out


def write_png(path, img):
    """8-bit grayscale PNG of a [H,W] uint8 array (what PIL writes for mode 'L'; any decoder reads the same pixels)."""
    _write_png8(path, img, 0, [], "write_png")


def _write_png8(path, img, colour_type, extra_chunks, who):
    """one 8-bit sample per pixel (grayscale or palette index), filter type 0, one IDAT; extra_chunks: (tag, data) between IHDR and IDAT"""
    a = np.ascontiguousarray(img, dtype=np.uint8)
    if a.ndim != 2:
        raise ValueError("%s expects a 2-D uint8 array, got shape %r" % (who, a.shape))
    h, w = a.shape
    raw = np.empty((h, w + 1), dtype=np.uint8)
    raw[:, 0] = 0                       # filter type 0 (None) per scanline
    raw[:, 1:] = a

    def chunk(tag, data):
        body = tag + data
        return struct.pack(">I", len(data)) + body + struct.pack(">I", zlib.crc32(body) & 0xFFFFFFFF)

    png = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, colour_type, 0, 0, 0)) \
        + b"".join(chunk(t, d) for t, d in extra_chunks) + chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + chunk(b"IEND", b"")
    with open(path, "wb") as f:
        f.write(png)


def save_masks(fused_logits, paths):
    """Test-loop body of train_online.py:181-187 for a batch: one PNG per frame."""
    b = mask_bytes(fused_logits).cpu().numpy()
    for img, p in zip(b, paths):
        write_png(p, img)


def _logits_and_truth(logits, gts, threshold):
    """-> (logits fp32 contiguous, the ground truth likewise and on their device, the logit of ``threshold``)"""
    g.need_cuda(logits, "logits", "results")
    g.need_cuda(gts, "gts", "results")
    thr = _threshold_logit(threshold)
    x = logits.detach().float().contiguous()
    gt = gts.detach().to(device=x.device, dtype=torch.float32).contiguous()
    if gt.numel() != x.numel():
        raise ValueError("logits and ground truth differ in size: %r vs %r" % (tuple(x.shape), tuple(gt.shape)))
    return x, gt, thr


def _frames_of(x):
    """(N, H, W) of a stack of one-channel frames [N,..,H,W]"""
    if x.dim() < 3:
        raise ValueError("expected N frames of H x W, got shape %r" % (tuple(x.shape),))
    n, h, w = int(x.shape[0]), int(x.shape[-2]), int(x.shape[-1])
    if x.numel() != n * h * w:
        raise ValueError("expected one channel per frame, got shape %r" % (tuple(x.shape),))
    return n, h, w


def jaccard(logits, gts, threshold=0.5):
    """DAVIS region measure per frame: J = |P & G| / |P | G| with P = sigmoid(logit) > threshold, G = gt > 0.5
    (J = 1 when both are empty).  logits, gts: CUDA tensors of N frames."""
    x, gt, thr = _logits_and_truth(logits, gts, threshold)
    n = x.shape[0]
    counts = torch.empty(2 * n, device=x.device, dtype=torch.int64)
    g.call("mask_iou_counts", x.device, g.ptr(x), g.ptr(gt), g.ptr(counts), x.numel() // n, n, thr)
    c = counts.cpu().numpy().reshape(n, 2)
    return [1.0 if u == 0 else float(i) / float(u) for i, u in c]


def davis_statistics(js):
    """mean, recall (fraction of frames with J > 0.5) and decay (mean of the first quarter minus mean of the last
    quarter of the frames) of a sequence's per-frame J, the three numbers DAVIS reports for the region measure."""
    j = np.asarray(js, dtype=np.float64)
    if j.size == 0:
        raise ValueError("no frames")
    bins = np.array_split(np.arange(j.size), 4) if j.size >= 4 else [np.arange(j.size)] * 4
    decay = float(j[bins[0]].mean() - j[bins[3]].mean()) if bins[0].size and bins[3].size else 0.0
    return {"mean": float(j.mean()), "recall": float((j > 0.5).mean()), "decay": decay}


def boundary_radius(h, w, bound_th=0.008):
    """Matching radius in pixels of the DAVIS boundary measure: ``bound_th`` itself when it is >= 1, otherwise
    ceil(bound_th * image diagonal) (854x480 -> 8, 1920x1080 -> 18)."""
    if bound_th >= 1:
        return int(bound_th)
    return int(math.ceil(bound_th * math.sqrt(float(h) * h + float(w) * w)))


def f_measure(n_fb, n_gb, fb_match, gb_match):
    """DAVIS contour accuracy F from the four boundary counts: harmonic mean of precision fb_match / n_fb and recall
    gb_match / n_gb; an empty boundary on one side scores that side 1 and the other 0, two empty boundaries score 1."""
    n_fb, n_gb = int(n_fb), int(n_gb)
    if n_fb == 0 and n_gb > 0:
        precision, recall = 1.0, 0.0
    elif n_fb > 0 and n_gb == 0:
        precision, recall = 0.0, 1.0
    elif n_fb == 0 and n_gb == 0:
        precision, recall = 1.0, 1.0
    else:
        precision, recall = float(fb_match) / float(n_fb), float(gb_match) / float(n_gb)
    if precision + recall == 0:
        return 0.0
    return 2.0 * precision * recall / (precision + recall)


def _jf_inputs(logits, gts, threshold):
    """jaccard's argument handling -> (logits [N,..,H,W] fp32 contiguous, gts likewise, N, H, W, logit threshold)"""
    x, gt, thr = _logits_and_truth(logits, gts, threshold)
    return (x, gt) + _frames_of(x) + (thr,)


def _boundary_ws(n, h, w, device, ws=None):
    return g.workspace(lib().osvos_boundary_ws_bytes(n, h, w), device, ws, "%d frames of %d x %d" % (n, h, w), "results", dtype=torch.int64)


def _enqueue_jf(x, gt, n, h, w, thr, radius, ws, counts_ptr):
    g.call("mask_jf_counts", x.device, g.ptr(x), g.ptr(gt), g.ptr(ws), C.c_void_p(counts_ptr), n, h, w, thr, radius, 0)


def _scores(rows):
    js = [1.0 if u == 0 else float(i) / float(u) for i, u in rows[:, :2]]
    fs = [f_measure(*r) for r in rows[:, 2:]]
    return js, fs


def boundary_f(logits, gts, threshold=0.5, bound_th=0.008):
    """DAVIS contour accuracy per frame: F of the boundaries of P = sigmoid(logit) > threshold and G = gt > 0.5, matched within
    ``boundary_radius(H, W, bound_th)`` pixels.  logits, gts: CUDA tensors of N frames (the arguments of ``jaccard``)."""
    x, gt, n, h, w, thr = _jf_inputs(logits, gts, threshold)
    ws = _boundary_ws(n, h, w, x.device)
    counts = torch.empty((n, 6), device=x.device, dtype=torch.int64)
    _enqueue_jf(x, gt, n, h, w, thr, boundary_radius(h, w, bound_th), ws, counts.data_ptr())
    return _scores(counts.cpu().numpy())[1]


class SequenceEvaluator(object):
    """J and F of a whole sequence with one host synchronisation: ``add`` enqueues the count kernels of a batch into a count table
    that lives on the device (nothing is read back, nothing waits), ``per_frame`` / ``summary`` copy the table to the host once.
    Frames of different sizes may follow each other (the matching radius is derived per call)."""

    CHUNK = 256      # frames the count table grows by

    def __init__(self, threshold=0.5, bound_th=0.008):
        _threshold_logit(threshold)
        self.threshold, self.bound_th = threshold, bound_th
        self.frames = 0
        self._table = None          # int64 [capacity, 6] on the device
        self._ws = None
        self._host = None           # (frames, rows) of the last read-back

    def add(self, logits, gts):
        x, gt, n, h, w, thr = _jf_inputs(logits, gts, self.threshold)
        need = self.frames + n
        if self._table is None or self._table.device != x.device or need > self._table.shape[0]:
            if self._table is not None and self._table.device != x.device:
                raise ValueError("all frames of a sequence must live on one device")
            grown = torch.zeros(((need + self.CHUNK - 1) // self.CHUNK * self.CHUNK, 6), device=x.device, dtype=torch.int64)
            if self._table is not None:
                grown[:self.frames].copy_(self._table[:self.frames])      # (device to device, in stream order)
            self._table = grown
        self._ws = _boundary_ws(n, h, w, x.device, self._ws)
        _enqueue_jf(x, gt, n, h, w, thr, boundary_radius(h, w, self.bound_th), self._ws, self._table.data_ptr() + 48 * self.frames)
        self.frames = need

    def per_frame(self):
        """(js, fs): per-frame J and F of everything added so far (one device-to-host copy)."""
        if self.frames == 0:
            return [], []
        if self._host is None or self._host[0] != self.frames:
            self._host = (self.frames, self._table[:self.frames].cpu().numpy())
        return _scores(self._host[1])

    def summary(self):
        js, fs = self.per_frame()
        j, f = davis_statistics(js), davis_statistics(fs)
        return {"J": j, "F": f, "J&F": 0.5 * (j["mean"] + f["mean"]), "frames": self.frames}


# ---- multi-object sequences (DAVIS 2017) ---------------------------------------------------------------------------------------------

def merge_objects(logits, threshold=0.5):
    """logits: float32 CUDA tensor [K,N,H,W] or [K,N,1,H,W], the fused outputs of K per-object networks for N frames -> uint8 CUDA tensor
    [N,H,W]: per pixel the object (1..K) with the highest logit -- the lowest index on a tie, a NaN never wins -- or 0 (background) when
    that logit does not exceed the one of ``threshold``.  Decided on the logits: no sigmoid is computed."""
    g.need_cuda(logits, "logits", "results")
    thr = _threshold_logit(threshold)
    x = logits.detach().float().contiguous()
    if x.dim() == 5 and x.shape[2] == 1:
        x = x[:, :, 0]
    if x.dim() != 4:
        raise ValueError("expected K objects x N frames of H x W, got shape %r" % (tuple(logits.shape),))
    k, n, h, w = [int(v) for v in x.shape]
    if not 1 <= k <= MAX_OBJECTS:
        raise ValueError("%d objects; the library is built for 1..%d" % (k, MAX_OBJECTS))
    out = torch.empty((n, h, w), device=x.device, dtype=torch.uint8)
    g.call("merge_objects", x.device, g.ptr(x), g.ptr(out), n, k, h, w, thr)
    return out


def davis_palette():
    """The 256 x 3 uint8 PASCAL-VOC colour map the DAVIS 2017 annotations carry: bit b of the index goes, three bits at a time, to bit
    7, 6, .. of red, green and blue (0 black, 1 (128,0,0), 2 (0,128,0), 3 (128,128,0), 4 (0,0,128), ...)."""
    pal = np.zeros((256, 3), dtype=np.uint8)
    for i in range(256):
        c = i
        for j in range(8):
            for ch in range(3):
                pal[i, ch] |= ((c >> ch) & 1) << (7 - j)
            c >>= 3
    return pal


def write_indexed_png(path, labels, palette=None):
    """8-bit indexed PNG (colour type 3 + PLTE) of a [H,W] uint8 label map; palette: [n <= 256, 3] uint8, default ``davis_palette()``."""
    pal = np.ascontiguousarray(davis_palette() if palette is None else palette, dtype=np.uint8)
    if pal.ndim != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= 256:
        raise ValueError("palette must be [1..256, 3] uint8, got shape %r" % (pal.shape,))
    a = np.asarray(labels)
    if a.size and int(a.max()) >= pal.shape[0]:
        raise ValueError("label %d has no palette entry (%d entries)" % (int(a.max()), pal.shape[0]))
    _write_png8(path, a, 3, [(b"PLTE", pal.tobytes())], "write_indexed_png")


def save_label_maps(labels, paths):
    """One indexed PNG per frame of a uint8 [N,H,W] label tensor (one byte per pixel crosses PCIe, in one copy)."""
    b = labels.cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    if b.ndim != 3 or len(paths) != b.shape[0]:
        raise ValueError("expected [N,H,W] labels and N paths, got shape %r and %d paths" % (b.shape, len(paths)))
    pal = davis_palette()
    for img, p in zip(b, paths):
        write_indexed_png(p, img, pal)


class MultiObjectEvaluator(object):
    """J and F per object of a multi-object sequence, ``SequenceEvaluator``'s way: ``add`` takes uint8 label maps (prediction and ground
    truth, ids 1..n_objects; 0 and larger ids belong to no object), enqueues the count kernels into a device table [frames, n_objects, 6]
    and reads nothing back; ``per_object`` / ``summary`` copy the table to the host once.  One bitmap workspace serves every ``add``: call
    them all on one stream (or order the streams yourself), as the kernels of two calls must not overlap."""

    CHUNK = 256      # frames the count table grows by

    def __init__(self, n_objects, bound_th=0.008):
        if not 1 <= int(n_objects) <= MAX_OBJECTS:
            raise ValueError("%r objects; the library is built for 1..%d" % (n_objects, MAX_OBJECTS))
        self.n_objects, self.bound_th = int(n_objects), bound_th
        self.frames = 0
        self._table = None          # int64 [capacity, n_objects, 6] on the device
        self._ws = None
        self._host = None           # (frames, table) of the last read-back

    def add(self, pred_labels, gt_labels):
        g.need_cuda(pred_labels, "pred_labels", "results")
        g.need_cuda(gt_labels, "gt_labels", "results")
        if pred_labels.dtype != torch.uint8 or gt_labels.dtype != torch.uint8:
            raise ValueError("label maps are uint8 tensors, got %s and %s" % (pred_labels.dtype, gt_labels.dtype))
        p = pred_labels.detach().contiguous()
        gt = gt_labels.detach().to(device=p.device).contiguous()
        if p.dim() < 2 or gt.numel() != p.numel():
            raise ValueError("prediction and ground truth differ in size: %r vs %r" % (tuple(pred_labels.shape), tuple(gt_labels.shape)))
        h, w = int(p.shape[-2]), int(p.shape[-1])
        n = p.numel() // (h * w)
        k = self.n_objects
        if n * k > 65535:
            raise ValueError("%d frames x %d objects in one call; add at most %d frames at a time" % (n, k, 65535 // k))
        need = self.frames + n
        if self._table is None or need > self._table.shape[0]:
            grown = torch.zeros(((need + self.CHUNK - 1) // self.CHUNK * self.CHUNK, k, 6), device=p.device, dtype=torch.int64)
            if self._table is not None:
                grown[:self.frames].copy_(self._table[:self.frames])      # (device to device, in stream order)
            self._table = grown
        if self._table.device != p.device:
            raise ValueError("all frames of a sequence must live on one device")
        self._ws = g.workspace(lib().osvos_labels_jf_ws_bytes(n, k, h, w), p.device, self._ws, "%d frames x %d objects of %d x %d" % (n, k, h, w),
                               "results", dtype=torch.int64)
        g.call("labels_jf_counts", p.device, g.ptr(p), g.ptr(gt), g.ptr(self._ws), C.c_void_p(self._table.data_ptr() + 48 * k * self.frames), n, k, h, w,
               boundary_radius(h, w, self.bound_th), 0)
        self.frames = need

    def _counts(self):
        """host int64 [frames, n_objects, 6] (one device-to-host copy per new state of the table)"""
        if self._host is None or self._host[0] != self.frames:
            self._host = (self.frames, self._table[:self.frames].cpu().numpy())
        return self._host[1]

    def per_object(self):
        """[(js, fs) for object 1..n_objects]: per-frame J and F of everything added so far (one device-to-host copy)."""
        if self.frames == 0:
            return [([], []) for _ in range(self.n_objects)]
        c = self._counts()
        return [_scores(c[:, k]) for k in range(self.n_objects)]

    def summary(self, exclude_ends=False):
        """Per object the DAVIS statistics of J and F and their J&F; 'J', 'F' and 'J&F' of the sequence are the means over the objects of
        the per-object means.  exclude_ends: leave out the first and the last frame (the DAVIS 2017 semi-supervised protocol: the first
        frame is given, the last one is not scored)."""
        if self.frames < (3 if exclude_ends else 1):
            raise ValueError("summary(exclude_ends=%s) needs at least %d frames, %d were added" % (bool(exclude_ends), 3 if exclude_ends else 1, self.frames))
        objs = []
        for js, fs in self.per_object():
            if exclude_ends:
                js, fs = js[1:-1], fs[1:-1]
            j, f = davis_statistics(js), davis_statistics(fs)
            objs.append({"J": j, "F": f, "J&F": 0.5 * (j["mean"] + f["mean"])})
        jm = float(np.mean([o["J"]["mean"] for o in objs]))
        fm = float(np.mean([o["F"]["mean"] for o in objs]))
        return {"objects": objs, "J": jm, "F": fm, "J&F": 0.5 * (jm + fm), "frames": self.frames - 2 if exclude_ends else self.frames}


# ---- connected components of the mask: clean-up and tracking ---------------------------------------------------------------------------

def _component_inputs(logits, threshold, connectivity):
    """_jf_inputs' argument handling without a ground truth -> (logits fp32 contiguous, N, H, W, logit threshold)"""
    thr = _threshold_logit(threshold)
    if connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8, got %r" % (connectivity,))
    g.need_cuda(logits, "logits", "results")
    x = logits.detach().float().contiguous()
    return (x,) + _frames_of(x) + (thr,)


def _components_ws(n, h, w, device, ws=None):
    return g.workspace(lib().osvos_components_ws_bytes(n, h, w), device, ws,
                       "%d frames of %d x %d (the library takes 1..65535 frames of fewer than 2^31 - 1 pixels)" % (n, h, w), "results", dtype=torch.int64)


def _enqueue_components(x, n, h, w, thr, connectivity, ws):
    labels = torch.empty((n, h, w), device=x.device, dtype=torch.int32)
    area = torch.empty((n, h, w), device=x.device, dtype=torch.int32)
    stats = torch.empty((n, 4), device=x.device, dtype=torch.int64)
    g.call("mask_components", x.device, g.ptr(x), g.ptr(labels), g.ptr(area), g.ptr(stats), g.ptr(ws), n, h, w, thr, connectivity)
    return labels, area, stats


def components(logits, threshold=0.5, connectivity=8):
    """Connected components of P = sigmoid(logit) > threshold per frame.  logits: CUDA tensor [N,1,H,W] or [N,H,W] -> CUDA tensors
    (labels int32 [N,H,W]: 0 off P, else 1 + the lowest flat index y W + x of the pixel's component; area int32 [N,H,W]: the component's pixel
    count at that root pixel, 0 elsewhere; stats int64 [N,4]: components, |P|, largest area, label of the largest -- lowest on a tie)."""
    x, n, h, w, thr = _component_inputs(logits, threshold, connectivity)
    return _enqueue_components(x, n, h, w, thr, connectivity, _components_ws(n, h, w, x.device))


def _seed_bytes(seed, device, frames, h, w):
    g.need_cuda(seed, "seed", "results")
    s = seed.detach().to(device=device)
    s = s.contiguous() if s.dtype == torch.uint8 else (s != 0).to(torch.uint8).contiguous()
    if s.numel() != frames * h * w or tuple(s.shape[-2:]) != (h, w):
        raise ValueError("seed of shape %r for %d frame(s) of %d x %d" % (tuple(seed.shape), frames, h, w))
    return s


def _enqueue_select(x, labels, area, stats, seed, chain, seed_radius, min_area, keep_largest, fill, thr, ws, n, h, w):
    out = torch.empty_like(x)
    kept = torch.empty((n, h, w), device=x.device, dtype=torch.uint8)
    g.call("components_select", x.device, g.ptr(x), g.ptr(labels), g.ptr(area), g.ptr(stats), g.ptr(seed), 1 if chain else 0, int(seed_radius),
           int(min_area), 1 if keep_largest else 0, float(fill), g.ptr(out), g.ptr(kept), g.ptr(ws), n, h, w, thr)
    return out, kept


def _select_arguments(seed_radius, min_area, fill, thr):
    if not 0 <= int(seed_radius) <= BOUNDARY_MAX_RADIUS:
        raise ValueError("seed_radius must be 0..%d pixels, got %r" % (BOUNDARY_MAX_RADIUS, seed_radius))
    if int(min_area) < 0:
        raise ValueError("min_area must not be negative, got %r" % (min_area,))
    if fill != fill or not float(np.float32(fill)) <= float(np.float32(thr)):
        raise ValueError("fill must be a number at or below the threshold's logit %g, got %r" % (thr, fill))


def filter_components(logits, threshold=0.5, connectivity=8, min_area=0, keep_largest=False, seed=None, seed_radius=0, chain=False,
                      fill=float('-inf')):
    """Drop connected components of the thresholded mask.  A component is kept when it has at least ``min_area`` pixels, is the largest of its
    frame (``keep_largest``; the lowest label on a tie) and passes the seed test: no ``seed``, an all-zero seed map (the object was lost, so
    everything passes), or a pixel within ``seed_radius`` pixels (a disk; 0 = overlap) of a non-zero seed pixel.  seed: uint8, bool or float
    CUDA tensor, [N,H,W] -- one map per frame -- or with ``chain`` [H,W] / [1,H,W], the seed of frame 0; frame n > 0 is then seeded by what
    was kept of frame n - 1.  -> (logits in the shape they came in, with ``fill`` at the foreground pixels of dropped components;
    kept uint8 [N,H,W])."""
    x, n, h, w, thr = _component_inputs(logits, threshold, connectivity)
    _select_arguments(seed_radius, min_area, fill, thr)
    if chain and seed is None:
        raise ValueError("chain needs the seed of the first frame")
    s = None if seed is None else _seed_bytes(seed, x.device, 1 if chain else n, h, w)
    ws = _components_ws(n, h, w, x.device)
    labels, area, stats = _enqueue_components(x, n, h, w, thr, connectivity, ws)
    out, kept = _enqueue_select(x, labels, area, stats, s, chain, seed_radius, min_area, keep_largest, fill, thr, ws, n, h, w)
    return out.view(logits.shape), kept


class ComponentTracker(object):
    """OSVOS segments every frame on its own; its typical failure is a false-positive blob far from the object.  The tracker keeps, frame after
    frame, the components that touch what was kept of the previous frame dilated by ``radius`` pixels, starting from the annotation of
    frame 0 (``first_mask`` [H,W] or [1,H,W], non-zero = object); when nothing was kept the next frame passes whole, so the object can be
    found again.  ``__call__`` takes a batch of consecutive frames and returns the filtered logits (dropped pixels at -inf); it enqueues
    only.  The last kept map, the workspace and the running counts live on the device; ``summary`` reads the counts back, once.  Call it on
    one stream (or order the streams yourself): one workspace serves every call.  ``seed`` is the kept map the next call starts from, uint8
    [1,H,W]: read it, move it (``flow.MotionCompensator.warp``) and assign it back when the object moves farther than ``radius`` a frame."""

    def __init__(self, first_mask, radius, threshold=0.5, connectivity=8, min_area=0):
        g.need_cuda(first_mask, "first_mask", "results")
        _threshold_logit(threshold)
        if connectivity not in (4, 8):
            raise ValueError("connectivity must be 4 or 8, got %r" % (connectivity,))
        m = first_mask.detach()
        if m.dim() == 3 and m.shape[0] == 1:
            m = m[0]
        if m.dim() != 2:
            raise ValueError("first_mask must be [H,W] or [1,H,W], got shape %r" % (tuple(first_mask.shape),))
        self.h, self.w = int(m.shape[0]), int(m.shape[1])
        self.radius, self.threshold, self.connectivity, self.min_area = int(radius), threshold, connectivity, int(min_area)
        _select_arguments(self.radius, self.min_area, float('-inf'), 0.0)
        self._seed = _seed_bytes(m, m.device, 1, self.h, self.w).view(1, self.h, self.w)
        self._counts = torch.zeros(3, device=m.device, dtype=torch.int64)      # components seen, components kept, frames
        self._ws = None
        self._host = None

    def __call__(self, logits):
        x, n, h, w, thr = _component_inputs(logits, self.threshold, self.connectivity)
        if (h, w) != (self.h, self.w):
            raise ValueError("frames of %d x %d follow a first mask of %d x %d" % (h, w, self.h, self.w))
        if x.device != self._seed.device:
            raise ValueError("all frames of a sequence must live on one device")
        self._ws = _components_ws(n, h, w, x.device, self._ws)
        labels, area, stats = _enqueue_components(x, n, h, w, thr, self.connectivity, self._ws)
        out, kept = _enqueue_select(x, labels, area, stats, self._seed, True, self.radius, self.min_area, False, float('-inf'), thr, self._ws, n, h, w)
        self._seed = kept[n - 1:n]
        self._counts[0] += stats[:, 0].sum()
        self._counts[1] += ((area > 0) & (kept != 0)).sum()                    # a component's root pixel carries its area
        self._counts[2] += n
        self._host = None
        return out.view(logits.shape)

    @property
    def seed(self):
        """the uint8 [1,H,W] map (non-zero = kept) the next frame's components are tested against"""
        return self._seed

    @seed.setter
    def seed(self, value):
        if not torch.is_tensor(value) or tuple(value.shape) != (1, self.h, self.w) or value.device != self._seed.device:
            raise ValueError("seed must be a [1,%d,%d] tensor on %s, got %r" % (self.h, self.w, self._seed.device,
                                                                              tuple(value.shape) if torch.is_tensor(value) else value))
        self._seed = _seed_bytes(value, value.device, 1, self.h, self.w).view(1, self.h, self.w)

    def summary(self):
        """{'seen', 'kept', 'frames'}: components met, components kept, frames passed so far (one device-to-host copy)."""
        if self._host is None:
            self._host = [int(v) for v in self._counts.cpu().numpy()]
        return {"seen": self._host[0], "kept": self._host[1], "frames": self._host[2]}


# ---- distance maps ----------------------------------------------------------------------------------------------------------------------

def mask_bytes_nhw(mask, who, module="results"):
    """a mask tensor [N,1,H,W], [N,H,W] or [H,W] (uint8, bool or float; non-zero = set) -> (uint8 contiguous [N,H,W], N, H, W), for the
    distance kernels: 1..65535 frames with sides of 1..SQDIST_MAX_SIDE.  ``who``: the calling function, for the messages"""
    g.need_cuda(mask, who + "'s mask", module)
    m, n, h, w = g.planes(mask.detach(), who + "'s mask")
    if not (1 <= n <= 65535 and 1 <= h <= SQDIST_MAX_SIDE and 1 <= w <= SQDIST_MAX_SIDE):
        raise ValueError("%s: %d frames of %d x %d: the library takes 1..65535 frames with sides of 1..%d" % (who, n, h, w, SQDIST_MAX_SIDE))
    return (m if m.dtype == torch.uint8 else (m != 0).to(torch.uint8)).view(n, h, w), n, h, w


def distance_map(mask, invert=False):
    """Exact squared Euclidean distance of every pixel to the nearest set pixel of its frame (``invert``: to the nearest pixel that is NOT
    set): int32 CUDA tensor [N,H,W], ``_lib.SQDIST_NONE`` everywhere in a frame without such a pixel (``osvos_mask_sqdist``).  Enqueued only."""
    m, n, h, w = mask_bytes_nhw(mask, "distance_map")
    out = torch.empty((n, h, w), device=m.device, dtype=torch.int32)
    ws = g.workspace(lib().osvos_mask_sqdist_ws_bytes(n, h, w), m.device, what="%d frames of %d x %d" % (n, h, w), prefix="results", dtype=torch.int32)
    g.call("mask_sqdist", m.device, g.ptr(m), 1 if invert else 0, g.ptr(out), n, h, w, g.ptr(ws))
    return out
