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
import math

import numpy as np
import torch

from . import _glue as g
from ._lib import CRF_MAX_ITERS, CRF_MAX_RADIUS, CRF_MAX_REACH

MAX_SIDE = 16384


def check_window(radius, dilation, iters=0):
    """ValueError unless (radius, dilation, iters) is a window osvos_crf_refine takes"""
    for name, v, lo, hi in (("radius", radius, 0, CRF_MAX_RADIUS), ("dilation", dilation, 1, None), ("iters", iters, 0, CRF_MAX_ITERS)):
        g.check_int(name, v, lo, hi, "crf")
    if radius * dilation > CRF_MAX_REACH:
        raise ValueError("crf: radius %d x dilation %d reaches %d pixels (at most %d)" % (radius, dilation, radius * dilation, CRF_MAX_REACH))


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


def refine_raw(logits, frames_u8, coeffs, iters, radius, dilation, init=None, out=None, ws=None):
    """one osvos_crf_refine call with the five coefficients given; ws: a float32 CUDA tensor of at least N H W elements, or None"""
    check_window(radius, dilation, iters)
    coeffs = tuple(float(c) for c in coeffs)
    if len(coeffs) != 5 or not all(math.isfinite(c) and c >= 0 for c in coeffs):
        raise ValueError("crf: five finite coefficients >= 0 (w_a, w_s, a_s, a_c, g_s), got %r" % (coeffs,))
    g.need_cuda(logits, "logits", "refine")
    u, n, h, w = g.planes(logits, "logits", (torch.float32,), MAX_SIDE, dims=(3, 4))
    g.need_cuda(frames_u8, "frames_u8", "refine")
    fr = g.frames(frames_u8, "frames_u8")
    if tuple(fr.shape) != (n, h, w, 3) or fr.device != u.device:
        raise ValueError("frames_u8 must be a uint8 [%d,%d,%d,3] tensor on the logits' device ([H,W,3] for one image), got %s %s"
                         % (n, h, w, fr.dtype, tuple(fr.shape)))
    z0 = None
    if init is not None:
        g.need_cuda(init, "init", "refine")
        z0 = g.planes(init, "init", (torch.float32,), dims=(3, 4))[0]
        if z0.numel() != u.numel() or tuple(z0.shape[-2:]) != (h, w) or z0.device != u.device:
            raise ValueError("init must hold one [%d,%d] map per image on the logits' device, got %s" % (h, w, tuple(z0.shape)))
    if out is None:
        out = torch.empty_like(u)
    else:
        g.need_cuda(out, "out", "refine")
        # (an iteration reads a neighbourhood of its source: the result cannot be written over it)
        g.out_buffer(out, torch.float32, u.shape, u.device, "the logits' device", alias=(("logits", u), ("init", z0)))
    if iters >= 2:
        if ws is None:
            ws = torch.empty(n * h * w, device=u.device, dtype=torch.float32)
        elif not (isinstance(ws, torch.Tensor) and ws.is_cuda and ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= n * h * w
                  and ws.device == u.device):
            raise ValueError("ws must be a contiguous float32 CUDA tensor of at least %d elements on the logits' device" % (n * h * w))
    g.call("crf_refine", u.device, g.ptr(u), g.ptr(z0), g.ptr(fr), g.ptr(out), g.ptr(ws) if iters >= 2 else None, n, h, w, int(iters), int(radius),
           int(dilation), *coeffs)
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
        g.need_cuda(logits, "logits", "refine")
        ws = None
        if self.iters >= 2:
            key = (logits.device, int(logits.numel()))
            ws = self._ws[key] = g.workspace(4 * max(1, int(logits.numel())), logits.device, self._ws.get(key), dtype=torch.float32)
        return refine_raw(logits, frames_u8, self.coeffs, self.iters, self.radius, self.dilation, init=init, out=out, ws=ws)


def parse_pair(text, n, what):
    """'4,1' -> (4.0, 1.0): n comma-separated finite numbers; ValueError otherwise"""
    return g.parse_numbers(text, (float,) * n, what, finite=True)
