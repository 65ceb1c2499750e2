"""Edge-aware refinement of a logit map against the frame it came from: mean field of a local two-label dense CRF (Potts compatibility,
ConvCRF-style window), on the device, logits in and logits out (``osvos_crf_refine``, csrc/crf.hip; the rule: include/osvos_hip.h).

    s_j = 2 sigmoid(z_j) - 1;    z_i <- u_i + sum_{j in window, j != i} (w_a exp(-(a_s ds + a_c dc)) + w_s exp(-g_s ds)) s_j

with ds the squared pixel distance and dc the squared BGR distance of the two pixels.  ``crf_coefficients`` turns weights in logits and
standard deviations in pixels / grey levels into the five numbers of the C ABI, ``crf_refine`` is one call, ``CrfRefiner`` a callable that
keeps its parameters and its workspace.  The result is a logit map of the input's shape: it goes wherever the network's output goes
(``results.ComponentTracker``, ``merge_objects``, ``save_masks``, the evaluators) and nothing is read back.

The default parameters are STARTING VALUES, NOT TUNED ON DAVIS (no dataset was at hand when this was written): tune them on a validation
split before quoting a score.
"""
import ctypes as C
import math

import numpy as np
import torch

from ._lib import CRF_MAX_ITERS, CRF_MAX_RADIUS, CRF_MAX_REACH, check, lib

MAX_SIDE = 16384


def check_window(radius, dilation, iters=0):
    """ValueError unless (radius, dilation, iters) is a window osvos_crf_refine takes"""
    for name, v in (("radius", radius), ("dilation", dilation), ("iters", iters)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("crf: %s must be an integer, got %r" % (name, v))
    if not 0 <= radius <= CRF_MAX_RADIUS:
        raise ValueError("crf: radius %d (0..%d)" % (radius, CRF_MAX_RADIUS))
    if dilation < 1:
        raise ValueError("crf: dilation %d (>= 1)" % dilation)
    if radius * dilation > CRF_MAX_REACH:
        raise ValueError("crf: radius %d x dilation %d reaches %d pixels (at most %d)" % (radius, dilation, radius * dilation, CRF_MAX_REACH))
    if not 0 <= iters <= CRF_MAX_ITERS:
        raise ValueError("crf: iters %d (0..%d)" % (iters, CRF_MAX_ITERS))


def window_offsets(radius, dilation):
    """squared lengths ds of the (2 radius + 1)^2 - 1 offsets of the window, float64"""
    r = np.arange(-radius, radius + 1, dtype=np.float64) * dilation
    ds = (r[:, None] ** 2 + r[None, :] ** 2).ravel()
    return np.delete(ds, ds.size // 2)


def crf_coefficients(radius, dilation, w_appearance, w_smooth, theta_alpha, theta_beta, theta_gamma, normalize=True):
    """-> (w_a, w_s, a_s, a_c, g_s) as the fp32 values osvos_crf_refine receives (Python floats).  a_s = 1 / (2 theta_alpha^2),
    a_c = 1 / (2 theta_beta^2), g_s = 1 / (2 theta_gamma^2): theta_alpha and theta_gamma in pixels, theta_beta in grey levels.  normalize:
    each weight is divided by the mass of its spatial kernel over the full window, sum_{d != 0} exp(-a_s ds) resp. exp(-g_s ds), so that
    |z - u| <= w_appearance + w_smooth logits whatever the window and the thetas are."""
    check_window(radius, dilation)
    vals = [float(v) for v in (w_appearance, w_smooth, theta_alpha, theta_beta, theta_gamma)]
    if not all(math.isfinite(v) for v in vals):
        raise ValueError("crf: weights and thetas must be finite, got %r" % (vals,))
    w_a, w_s, ta, tb, tg = vals
    if w_a < 0 or w_s < 0:
        raise ValueError("crf: weights must be >= 0, got %r and %r" % (w_a, w_s))
    if not (ta > 0 and tb > 0 and tg > 0):
        raise ValueError("crf: thetas must be > 0, got %r, %r and %r" % (ta, tb, tg))
    a_s, a_c, g_s = (float(np.float32(1.0 / (2.0 * t * t))) for t in (ta, tb, tg))
    if normalize and radius > 0:
        ds = window_offsets(radius, dilation)
        # (the masses are taken with the fp32 coefficients the kernel gets; a kernel narrower than the dilation has almost no mass: the
        #  quotient may overflow fp32, which is refused below)
        with np.errstate(divide="ignore", over="ignore"):
            w_a = float(w_a / np.exp(-a_s * ds).sum()) if w_a else 0.0
            w_s = float(w_s / np.exp(-g_s * ds).sum()) if w_s else 0.0
    out = tuple(float(np.float32(v)) for v in (w_a, w_s, a_s, a_c, g_s))
    if not all(math.isfinite(v) for v in out):
        raise ValueError("crf: the coefficients %r do not fit fp32 (a theta far below the dilation leaves its kernel no mass)" % (out,))
    return out


def _need_cuda(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("osvos_pytorch_amd.refine needs CUDA (ROCm) tensors (%s); there is no CPU fallback" % what)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _maps(t, what):
    """[N,1,H,W] or [N,H,W] float32 -> the contiguous tensor (same layout)"""
    _need_cuda(t, what)
    if t.dtype != torch.float32 or not (t.dim() == 3 or (t.dim() == 4 and t.shape[1] == 1)):
        raise ValueError("%s must be a float32 [N,1,H,W] or [N,H,W] tensor, got %s %s" % (what, t.dtype, tuple(t.shape)))
    return t.contiguous()


def refine_raw(logits, frames_u8, coeffs, iters, radius, dilation, init=None, out=None, ws=None):
    """one osvos_crf_refine call with the five coefficients given; ws: a float32 CUDA tensor of at least N H W elements, or None"""
    check_window(radius, dilation, iters)
    coeffs = tuple(float(c) for c in coeffs)
    if len(coeffs) != 5 or not all(math.isfinite(c) and c >= 0 for c in coeffs):
        raise ValueError("crf: five finite coefficients >= 0 (w_a, w_s, a_s, a_c, g_s), got %r" % (coeffs,))
    u = _maps(logits, "logits")
    n, h, w = int(u.shape[0]), int(u.shape[-2]), int(u.shape[-1])
    if n < 1 or not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError("logits of %s: N >= 1 and sides 1..%d" % (tuple(u.shape), MAX_SIDE))
    _need_cuda(frames_u8, "frames_u8")
    if frames_u8.dim() == 3:
        frames_u8 = frames_u8[None]
    if frames_u8.dtype != torch.uint8 or tuple(frames_u8.shape) != (n, h, w, 3) or frames_u8.device != u.device:
        raise ValueError("frames_u8 must be a uint8 [%d,%d,%d,3] tensor on the logits' device ([H,W,3] for one image), got %s %s"
                         % (n, h, w, frames_u8.dtype, tuple(frames_u8.shape)))
    frames_u8 = frames_u8.contiguous()
    z0 = None
    if init is not None:
        z0 = _maps(init, "init")
        if z0.numel() != u.numel() or tuple(z0.shape[-2:]) != (h, w) or z0.device != u.device:
            raise ValueError("init must hold one [%d,%d] map per image on the logits' device, got %s" % (h, w, tuple(z0.shape)))
    if out is None:
        out = torch.empty_like(u)
    else:
        _need_cuda(out, "out")
        if out.dtype != torch.float32 or tuple(out.shape) != tuple(u.shape) or not out.is_contiguous() or out.device != u.device:
            raise ValueError("out must be a contiguous float32 tensor of shape %s on the logits' device" % (tuple(u.shape),))
        if out.data_ptr() == u.data_ptr() or (z0 is not None and out.data_ptr() == z0.data_ptr()):
            raise ValueError("out must not be logits or init: an iteration reads a neighbourhood of its source")
    if iters >= 2:
        if ws is None:
            ws = torch.empty(n * h * w, device=u.device, dtype=torch.float32)
        elif not (isinstance(ws, torch.Tensor) and ws.is_cuda and ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= n * h * w
                  and ws.device == u.device):
            raise ValueError("ws must be a contiguous float32 CUDA tensor of at least %d elements on the logits' device" % (n * h * w))
    vp = C.c_void_p
    with torch.cuda.device(u.device):
        check(lib().osvos_crf_refine(vp(u.data_ptr()), vp(z0.data_ptr()) if z0 is not None else None, vp(frames_u8.data_ptr()), vp(out.data_ptr()),
                                     vp(ws.data_ptr()) if iters >= 2 else None, n, h, w, int(iters), int(radius), int(dilation), *coeffs,
                                     _stream()), "crf_refine")
    return out


def crf_refine(logits, frames_u8, iters=5, radius=5, dilation=3, w_appearance=4.0, w_smooth=1.0, theta_alpha=8.0, theta_beta=13.0,
               theta_gamma=3.0, normalize=True, init=None, out=None):
    """logits: float32 CUDA [N,1,H,W] or [N,H,W]; frames_u8: the decoded uint8 BGR frames [N,H,W,3] ([H,W,3] for N = 1) on the same device
    -> the refined logits, in the shape of ``logits``: ``iters`` mean-field steps over a (2 radius + 1)^2 window of every ``dilation``-th
    pixel, started at ``init`` (default: the logits).  Weights in logits, theta_alpha / theta_gamma in pixels, theta_beta in grey levels
    (``crf_coefficients``).  out: a contiguous float32 tensor of that shape to write into; it must not be ``logits`` or ``init``.

    The defaults are starting values, NOT tuned on DAVIS."""
    coeffs = crf_coefficients(radius, dilation, w_appearance, w_smooth, theta_alpha, theta_beta, theta_gamma, normalize)
    return refine_raw(logits, frames_u8, coeffs, iters, radius, dilation, init=init, out=out)


class CrfRefiner(object):
    """``CrfRefiner(...)(logits, frames_u8)``: crf_refine with the parameters fixed at construction (the coefficients are made once) and one
    workspace kept per (device, size).  The defaults are starting values, NOT tuned on DAVIS."""

    def __init__(self, iters=5, radius=5, dilation=3, w_appearance=4.0, w_smooth=1.0, theta_alpha=8.0, theta_beta=13.0, theta_gamma=3.0,
                 normalize=True):
        check_window(radius, dilation, iters)
        self.iters, self.radius, self.dilation = int(iters), int(radius), int(dilation)
        self.coeffs = crf_coefficients(radius, dilation, w_appearance, w_smooth, theta_alpha, theta_beta, theta_gamma, normalize)
        self._ws = {}

    def __call__(self, logits, frames_u8, init=None, out=None):
        _need_cuda(logits, "logits")
        ws = None
        if self.iters >= 2:
            key = (logits.device, int(logits.numel()))
            ws = self._ws.get(key)
            if ws is None:
                ws = self._ws[key] = torch.empty(max(1, int(logits.numel())), device=logits.device, dtype=torch.float32)
        return refine_raw(logits, frames_u8, self.coeffs, self.iters, self.radius, self.dilation, init=init, out=out, ws=ws)


def parse_pair(text, n, what):
    """'4,1' -> (4.0, 1.0): n comma-separated finite numbers; ValueError otherwise"""
    parts = [t.strip() for t in (text or "").split(",")]
    if len(parts) != n:
        raise ValueError("%s takes %d comma-separated numbers, got %r" % (what, n, text))
    try:
        vals = tuple(float(t) for t in parts)
    except ValueError:
        raise ValueError("%s takes %d comma-separated numbers, got %r" % (what, n, text))
    if not all(math.isfinite(v) for v in vals):
        raise ValueError("%s takes finite numbers, got %r" % (what, text))
    return vals
