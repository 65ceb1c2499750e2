"""Result writer and evaluator for the per-sequence test loop (reference train_online.py:181-189).

The reference turns the fused logit map into a probability (``1 / (1 + exp(-x))``), hands it to ``scipy.misc.imsave``
(scipy <= 1.1: min-max byte scaling, PIL mode 'L') and leaves the DAVIS evaluation to an external toolkit.  Here the
sigmoid + byte scaling run on the device (``osvos_mask_to_bytes``: one byte per pixel crosses PCIe instead of four),
the PNG is written by a small zlib encoder (no PIL / scipy dependency), and the two DAVIS measures -- region similarity J
(Jaccard index of the thresholded mask) and contour accuracy F (boundary precision / recall within a disk of 0.8 % of the
image diagonal) -- with their mean / recall / decay statistics and the headline J&F are computed from device-side integer
counts (``osvos_mask_iou_counts``, ``osvos_mask_jf_counts``); ``SequenceEvaluator`` keeps the counts of a whole sequence on
the device and reads them back once.
"""
import ctypes as C
import math
import struct
import zlib

import numpy as np
import torch

from ._lib import check, lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def mask_bytes(logits):
    """logits: float32 CUDA tensor [N,1,H,W] or [N,H,W] -> uint8 CUDA tensor [N,H,W] (imsave's byte image per frame)."""
    if not logits.is_cuda:
        raise RuntimeError("osvos_pytorch_amd.results needs CUDA (ROCm) tensors; there is no CPU fallback")
    x = logits.detach().float().contiguous()
    n = x.shape[0]
    count = x.numel() // n
    out = torch.empty((n,) + tuple(x.shape[-2:]), device=x.device, dtype=torch.uint8)
    scratch = torch.empty(2 * n, device=x.device, dtype=torch.int32)
    check(lib().osvos_mask_to_bytes(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(scratch.data_ptr()), count, n, _stream()),
          "mask_to_bytes")
    return out


def write_png(path, img):
    """8-bit grayscale PNG of a [H,W] uint8 array (what PIL writes for mode 'L'; any decoder reads the same pixels)."""
    a = np.ascontiguousarray(img, dtype=np.uint8)
    if a.ndim != 2:
        raise ValueError("write_png expects a 2-D uint8 array, got shape %r" % (a.shape,))
    h, w = a.shape
    raw = np.empty((h, w + 1), dtype=np.uint8)
    raw[:, 0] = 0                       # filter type 0 (None) per scanline
    raw[:, 1:] = a

    def chunk(tag, data):
        body = tag + data
        return struct.pack(">I", len(data)) + body + struct.pack(">I", zlib.crc32(body) & 0xFFFFFFFF)

    png = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) \
        + chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + chunk(b"IEND", b"")
    with open(path, "wb") as f:
        f.write(png)


def save_masks(fused_logits, paths):
    """Test-loop body of train_online.py:181-187 for a batch: one PNG per frame."""
    b = mask_bytes(fused_logits).cpu().numpy()
    for img, p in zip(b, paths):
        write_png(p, img)


def jaccard(logits, gts, threshold=0.5):
    """DAVIS region measure per frame: J = |P & G| / |P | G| with P = sigmoid(logit) > threshold, G = gt > 0.5
    (J = 1 when both are empty).  logits, gts: CUDA tensors of N frames."""
    if not (logits.is_cuda and gts.is_cuda):
        raise RuntimeError("osvos_pytorch_amd.results needs CUDA (ROCm) tensors; there is no CPU fallback")
    if not 0.0 < threshold < 1.0:
        raise ValueError("threshold must be a probability in (0, 1)")
    x = logits.detach().float().contiguous()
    g = gts.detach().to(device=x.device, dtype=torch.float32).contiguous()
    if g.numel() != x.numel():
        raise ValueError("logits and ground truth differ in size: %r vs %r" % (tuple(x.shape), tuple(g.shape)))
    n = x.shape[0]
    counts = torch.empty(2 * n, device=x.device, dtype=torch.int64)
    thr = float(np.log(threshold / (1.0 - threshold)))
    check(lib().osvos_mask_iou_counts(C.c_void_p(x.data_ptr()), C.c_void_p(g.data_ptr()), C.c_void_p(counts.data_ptr()), x.numel() // n, n, thr,
                                      _stream()), "mask_iou_counts")
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
    if not (logits.is_cuda and gts.is_cuda):
        raise RuntimeError("osvos_pytorch_amd.results needs CUDA (ROCm) tensors; there is no CPU fallback")
    if not 0.0 < threshold < 1.0:
        raise ValueError("threshold must be a probability in (0, 1)")
    x = logits.detach().float().contiguous()
    g = gts.detach().to(device=x.device, dtype=torch.float32).contiguous()
    if g.numel() != x.numel():
        raise ValueError("logits and ground truth differ in size: %r vs %r" % (tuple(x.shape), tuple(g.shape)))
    if x.dim() < 3:
        raise ValueError("expected N frames of H x W, got shape %r" % (tuple(x.shape),))
    n, h, w = int(x.shape[0]), int(x.shape[-2]), int(x.shape[-1])
    if x.numel() != n * h * w:
        raise ValueError("expected one channel per frame, got shape %r" % (tuple(x.shape),))
    return x, g, n, h, w, float(np.log(threshold / (1.0 - threshold)))


def _enqueue_jf(x, g, n, h, w, thr, radius, ws, counts_ptr):
    check(lib().osvos_mask_jf_counts(C.c_void_p(x.data_ptr()), C.c_void_p(g.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_void_p(counts_ptr),
                                     n, h, w, thr, radius, 0, _stream()), "mask_jf_counts")


def _scores(rows):
    js = [1.0 if u == 0 else float(i) / float(u) for i, u in rows[:, :2]]
    fs = [f_measure(*r) for r in rows[:, 2:]]
    return js, fs


def boundary_f(logits, gts, threshold=0.5, bound_th=0.008):
    """DAVIS contour accuracy per frame: F of the boundaries of P = sigmoid(logit) > threshold and G = gt > 0.5, matched within
    ``boundary_radius(H, W, bound_th)`` pixels.  logits, gts: CUDA tensors of N frames (the arguments of ``jaccard``)."""
    x, g, n, h, w, thr = _jf_inputs(logits, gts, threshold)
    ws = torch.empty(lib().osvos_boundary_ws_bytes(n, h, w) // 8, device=x.device, dtype=torch.int64)
    counts = torch.empty((n, 6), device=x.device, dtype=torch.int64)
    _enqueue_jf(x, g, n, h, w, thr, boundary_radius(h, w, bound_th), ws, counts.data_ptr())
    return _scores(counts.cpu().numpy())[1]


class SequenceEvaluator(object):
    """J and F of a whole sequence with one host synchronisation: ``add`` enqueues the count kernels of a batch into a count table
    that lives on the device (nothing is read back, nothing waits), ``per_frame`` / ``summary`` copy the table to the host once.
    Frames of different sizes may follow each other (the matching radius is derived per call)."""

    CHUNK = 256      # frames the count table grows by

    def __init__(self, threshold=0.5, bound_th=0.008):
        if not 0.0 < threshold < 1.0:
            raise ValueError("threshold must be a probability in (0, 1)")
        self.threshold, self.bound_th = threshold, bound_th
        self.frames = 0
        self._table = None          # int64 [capacity, 6] on the device
        self._ws = None
        self._host = None           # (frames, rows) of the last read-back

    def add(self, logits, gts):
        x, g, n, h, w, thr = _jf_inputs(logits, gts, self.threshold)
        need = self.frames + n
        if self._table is None or self._table.device != x.device or need > self._table.shape[0]:
            if self._table is not None and self._table.device != x.device:
                raise ValueError("all frames of a sequence must live on one device")
            grown = torch.zeros(((need + self.CHUNK - 1) // self.CHUNK * self.CHUNK, 6), device=x.device, dtype=torch.int64)
            if self._table is not None:
                grown[:self.frames].copy_(self._table[:self.frames])      # (device to device, in stream order)
            self._table = grown
        words = lib().osvos_boundary_ws_bytes(n, h, w) // 8
        if self._ws is None or self._ws.numel() < words:
            self._ws = torch.empty(words, device=x.device, dtype=torch.int64)
        _enqueue_jf(x, g, n, h, w, thr, boundary_radius(h, w, self.bound_th), self._ws, self._table.data_ptr() + 48 * self.frames)
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
