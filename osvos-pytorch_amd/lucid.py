"""Lucid first-frame synthesis ("lucid data dreaming"): more training samples out of the one annotated frame, on the device
(``osvos_lucid_inpaint`` / ``osvos_lucid_compose`` / ``osvos_lucid_compose_ex``, csrc/lucid.hip; the rule: include/osvos_hip.h).

    cut the object out, fill the hole (once per sequence), then per training sample move object and background by affines of their own,
    re-light both, and composite them again -- optionally with the object bent by a smooth displacement field (non-rigid deformation),
    partly hidden behind an ellipse of displaced background (an occluder), and with a band of void labels (-1) around the label's edges

Online fine-tuning otherwise sees its one frame only flipped, rotated and scaled as a whole (``augment.DeviceAugment``): the object never
moves against its background, is never lit differently from it, never changes shape, is never hidden, and what lies behind it is never
seen.  Integers only: the samples are exact and repeat bit for bit.  Everything stays on the device; ``LucidDream`` reads back four numbers
(the object's bounding box) once.

Left out: cubic lattices, premultiplied foreground colours.  The default parameters are STARTING VALUES, NOT TUNED ON DAVIS (no dataset
was at hand when this was written), and no accuracy claim is made for them.
"""
import ctypes as C
import math
import random

import numpy as np
import torch

from . import _glue as g
from ._lib import (LUCID_MAX_BAND, LUCID_MAX_BATCH, LUCID_MAX_CELL, LUCID_MAX_GAIN, LUCID_MAX_OCC_OFFSET, LUCID_MAX_OCC_RADIUS, LUCID_MAX_PASSES,
                   LUCID_MAX_RADIUS, LUCID_MAX_SIDE, LUCID_MIN_CELL, SQDIST_MAX_SIDE, lib)
from .augment import MEANVAL

MAX_GROW = 64               # largest --lucid-grow: pixels the hole reaches beyond the mask
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
NEUTRAL = (256, 256, 256, 0, 0, 0)


def check_lucid(p=0.0, grow=5, radius=2, passes=3, fg_shift=0.25, bg_shift=0.05, gain=0.2, offset=20, deform=0.0, occlude=0.0, band=0, cell=128):
    """ValueError unless the parameters of ``LucidDream`` (and the probability ``p`` of train_online.py --lucid) are inside their limits
    (host only)"""
    for name, v, lo, hi in (("grow", grow, 0, MAX_GROW), ("radius", radius, 1, LUCID_MAX_RADIUS), ("passes", passes, 0, LUCID_MAX_PASSES),
                            ("offset", offset, 0, 255), ("band", band, 0, LUCID_MAX_BAND), ("cell", cell, LUCID_MIN_CELL, LUCID_MAX_CELL)):
        g.check_int(name, v, lo, hi, "lucid")
    if cell & (cell - 1):
        raise ValueError("lucid: cell %d (a power of two in %d..%d)" % (cell, LUCID_MIN_CELL, LUCID_MAX_CELL))
    for name, v, hi in (("p", p, 1.0), ("fg_shift", fg_shift, 4.0), ("bg_shift", bg_shift, 1.0), ("gain", gain, 1.0), ("deform", deform, 1.0),
                        ("occlude", occlude, 1.0)):
        g.check_number(name, v, 0, hi, "lucid")


def field_shape(h, w, cell):
    """(GH, GW) of the deformation lattice of an h x w frame: control points every ``cell`` pixels, one row and one column past the last
    pixel's cell"""
    check_lucid(cell=cell)
    g.check_int("field_shape's h", h, 1, None, "lucid")
    g.check_int("field_shape's w", w, 1, None, "lucid")
    s = int(cell).bit_length() - 1
    return ((int(h) - 1) >> s) + 2, ((int(w) - 1) >> s) + 2


def affine_inverse(cx, cy, rot=0.0, sc=1.0, dx=0.0, dy=0.0, mirror=False):
    """The 6 float64 of the dst -> src affine of: (mirror about the vertical line through the pivot,) rotate by ``rot`` degrees and scale by
    ``sc`` about the pivot (cx, cy) -- the sense of cv2.getRotationMatrix2D, as ``augment.rotation_matrix_inverse`` -- then shift by (dx, dy).
    Identity arguments give exactly (1, 0, 0, 0, 1, 0); a pure integer shift gives exactly (1, 0, -dx, 0, 1, -dy)."""
    if not sc > 0:
        raise ValueError("lucid: scale %r (> 0)" % (sc,))
    a = float(rot) * math.pi / 180.0
    c, s = math.cos(a) / float(sc), math.sin(a) / float(sc)
    m0, m1, m3, m4 = c, -s, s, c
    if mirror:
        m0, m1 = -m0, -m1
    tx, ty = float(cx) + float(dx), float(cy) + float(dy)
    m = [m0, m1, float(cx) - m0 * tx - m1 * ty, m3, m4, float(cy) - m3 * tx - m4 * ty]
    return [v + 0.0 for v in m]                    # (-0.0 -> 0.0)


def _frame(t, what, max_side):
    """uint8 [H,W,3] -> the contiguous frame, [H,W,3]"""
    g.need_cuda(t, what, "lucid")
    return g.frames(t, what, max_side, batch=False)[0]


def _plane(t, like, what):
    g.need_cuda(t, what, "lucid")
    if t.dtype != torch.uint8 or tuple(t.shape) != tuple(like.shape[:2]) or t.device != like.device:
        raise ValueError("%s must be a uint8 %s tensor on the device of the frame, got %s %s" % (what, tuple(like.shape[:2]), t.dtype, tuple(t.shape)))
    return t.contiguous()


def inpaint(frame_u8, hole_u8, radius=2, passes=3, ws=None):
    """frame_u8: uint8 CUDA tensor [H,W,3] (BGR); hole_u8: uint8 [H,W], non-zero = to be filled -> uint8 [H,W,3]: every hole pixel filled
    with the colour of its nearest non-hole pixel (ties: the smaller row, then the smaller column), then ``passes`` box means of radius
    ``radius`` over the hole pixels.  Enqueued only."""
    check_lucid(radius=radius, passes=passes)
    f = _frame(frame_u8, "frame_u8", SQDIST_MAX_SIDE)
    hole = _plane(hole_u8, f, "hole_u8")
    h, w = int(f.shape[0]), int(f.shape[1])
    ws = g.workspace(lib().osvos_lucid_inpaint_ws_bytes(h, w, int(passes)), f.device, ws, "%d x %d with %d passes" % (h, w, passes), "lucid",
                     dtype=torch.int32)
    out = torch.empty_like(f)
    g.call("lucid_inpaint", f.device, g.ptr(f), g.ptr(hole), g.ptr(out), h, w, int(radius), int(passes), g.ptr(ws))
    return out


def compose(frame_u8, mask_u8, bg_u8, matrices, tones, meanval=MEANVAL, occluders=None, field=None, cell=64, band=0, ws=None):
    """frame_u8, bg_u8: uint8 CUDA tensors [H,W,3]; mask_u8: uint8 [H,W] (non-zero = object); matrices: [N][2][6] numbers, the dst -> src
    affines of (foreground, background) per sample (``affine_inverse``); tones: [N][2][6] integers (g_b, g_g, g_r, o_b, o_g, o_r), gains in Q8
    (256 = 1, 0..1024), offsets -255..255 -> (image float32 [N,3,H,W], gt float32 [N,1,H,W]) from one launch.  Enqueued only.

    The options go through ``osvos_lucid_compose_ex``; without any of them the call is ``osvos_lucid_compose`` as before.  ``occluders``:
    [N][6] integers (cx, cy, rx, ry, sx, sy) -- inside the ellipse the sample shows the background from (sx, sy) further on, label 0;
    rx = 0 or ry = 0: none in that sample.  ``field``: the foreground's displacement, int16 [N,GH,GW,2] = (dx, dy) in 1/32 pixel on a lattice
    of ``cell`` pixels (``field_shape``), a CUDA tensor or an array-like that is uploaded in one copy.  ``band`` 1..16: labels within that many
    pixels of a label edge are -1 (void; one more launch); ``ws``: a CUDA tensor to hold the label plane, allocated when missing or small."""
    f = _frame(frame_u8, "frame_u8", LUCID_MAX_SIDE)
    bg = _frame(bg_u8, "bg_u8", LUCID_MAX_SIDE)
    if bg.shape != f.shape or bg.device != f.device:
        raise ValueError("bg_u8 must match frame_u8, got %s and %s" % (tuple(bg.shape), tuple(f.shape)))
    mask = _plane(mask_u8, f, "mask_u8")
    m = np.ascontiguousarray(np.asarray(matrices, dtype=np.float64))
    t = np.asarray(tones)
    if m.ndim != 3 or m.shape[1:] != (2, 6) or not 1 <= m.shape[0] <= LUCID_MAX_BATCH:
        raise ValueError("lucid: matrices must be [N][2][6] with N 1..%d, got %s" % (LUCID_MAX_BATCH, m.shape))
    if t.shape != m.shape or not np.issubdtype(t.dtype, np.integer):
        raise ValueError("lucid: tones must be integers [%d][2][6], got %s %s" % (m.shape[0], t.dtype, t.shape))
    if not np.isfinite(m).all() or (np.abs(m[..., [0, 1, 3, 4]]) > 64).any() or (np.abs(m[..., [2, 5]]) > 2 ** 18).any():
        raise ValueError("lucid: matrix entries must be finite, |M0|, |M1|, |M3|, |M4| <= 64 and |M2|, |M5| <= 2^18")
    if (t[..., :3] < 0).any() or (t[..., :3] > LUCID_MAX_GAIN).any() or (np.abs(t[..., 3:]) > 255).any():
        raise ValueError("lucid: gains 0..%d (Q8), offsets -255..255" % LUCID_MAX_GAIN)
    t = np.ascontiguousarray(t.astype(np.int32))
    n, h, w = int(m.shape[0]), int(f.shape[0]), int(f.shape[1])
    image = torch.empty((n, 3, h, w), device=f.device, dtype=torch.float32)
    gt = torch.empty((n, 1, h, w), device=f.device, dtype=torch.float32)
    mean = (C.c_float * 3)(*meanval)
    vp = C.c_void_p
    if occluders is None and field is None and band == 0:
        g.call("lucid_compose", f.device, g.ptr(f), g.ptr(mask), g.ptr(bg), vp(m.ctypes.data), vp(t.ctypes.data), mean, g.ptr(image), g.ptr(gt), n, h, w)
        return image, gt
    g.check_int("band", band, 0, LUCID_MAX_BAND, "lucid")
    occ = None
    if occluders is not None:
        occ = np.asarray(occluders)
        if occ.shape != (n, 6) or not np.issubdtype(occ.dtype, np.integer):
            raise ValueError("lucid: occluders must be integers [%d][6], got %s %s" % (n, occ.dtype, occ.shape))
        if (occ[:, 2:4] < 0).any() or (occ[:, 2:4] > LUCID_MAX_OCC_RADIUS).any() or (np.abs(occ[:, [0, 1, 4, 5]]) > LUCID_MAX_OCC_OFFSET).any():
            raise ValueError("lucid: occluder radii 0..%d, |centre| and |offset| <= %d" % (LUCID_MAX_OCC_RADIUS, LUCID_MAX_OCC_OFFSET))
        occ = np.ascontiguousarray(occ.astype(np.int32))
    d = None
    if field is not None:
        check_lucid(cell=cell)
        want = (n,) + field_shape(h, w, cell) + (2,)
        if isinstance(field, torch.Tensor):
            if field.dtype != torch.int16 or tuple(field.shape) != want or field.device != f.device:
                raise ValueError("lucid: field must be an int16 %s tensor on the device of the frame, got %s %s" % (want, field.dtype, tuple(field.shape)))
            d = field.contiguous()
        else:
            a = np.asarray(field)
            if a.shape != want or not np.issubdtype(a.dtype, np.integer) or (a < -32768).any() or (a > 32767).any():
                raise ValueError("lucid: field must be int16 values %s, got %s %s" % (want, a.dtype, a.shape))
            d = torch.from_numpy(np.ascontiguousarray(a.astype(np.int16))).to(f.device)      # the one copy
        if d.data_ptr() % 4:
            raise ValueError("lucid: field must be 4-byte aligned")
    need = int(lib().osvos_lucid_compose_ex_ws_bytes(n, h, w, int(band)))
    ws = g.workspace(need, f.device, ws, dtype=torch.int64, align=8) if need else None      # (0: no band, no label plane)
    g.call("lucid_compose_ex", f.device, g.ptr(f), g.ptr(mask), g.ptr(bg), vp(m.ctypes.data), vp(t.ctypes.data),
           vp(occ.ctypes.data) if occ is not None else None, g.ptr(d), int(cell), int(band), mean, g.ptr(image), g.ptr(gt), n, h, w, g.ptr(ws))
    return image, gt


class LucidDream(object):
    """Lucid samples of one annotated frame.  At construction: the hole is ``results.distance_map(mask) <= grow^2`` (the mask grown by
    ``grow`` pixels), the frame is inpainted once, and the mask's bounding box is read back once (the foreground pivots about its centre;
    an empty mask pivots about the frame's centre).  Frame, mask and inpainted background stay on the device.

    ``draw()`` takes 13 numbers from Python's ``random``, in this order: ``random.random() < 0.5`` (mirror: both layers, each about its own
    pivot); foreground rotation, scale, shift x, shift y; background rotation, scale, shift x, shift y; foreground gain, foreground offset,
    background gain, background offset.  Rotation and scale are drawn as ``DeviceAugment`` draws them from ``rots`` / ``scales``; a shift is
    uniform in +-``fg_shift`` times the object box's side (+-``bg_shift`` times the frame's side); a gain is uniform in 1 +-``gain`` (all three
    channels alike, rounded to Q8), an offset a uniform integer in +-``offset`` grey levels.  With ``deform``, ``occlude`` and ``band`` off
    not one further number is drawn.

    Then, with ``deform`` > 0, 2 GH GW numbers (``field_shape(H, W, deform_cell)``), in the order lattice row gy, lattice column gx, dx then
    dy: a control point's displacement is ``round(4 deform_cell deform (2 u - 1))`` in 1/32 pixel, that is at most ``deform * deform_cell / 8``
    pixels -- neighbouring control points differ by at most a quarter of their spacing, so the bilinear map cannot fold.  Then, with
    ``occlude`` > 0, 7 numbers, always all seven: presence (``u < occlude``); the centre's x and y, ``round(x0 + u box_w)`` and
    ``round(y0 + u box_h)`` over the object's box; the semi-axes ``round((0.1 + 0.2 u) box_w)`` and ``round((0.1 + 0.2 u) box_h)``; the
    offset of the background shown in the ellipse, ``round((2 u - 1) W / 4)`` and ``round((2 u - 1) H / 4)``.  An absent occluder, or an
    empty mask, gives rx = 0 (all six numbers 0).  ``band`` > 0 draws nothing: labels within ``band`` pixels of a label edge are -1 (void).

    ``dream()`` -> {'image': [3,H,W], 'gt': [1,H,W]} as ``DeviceAugment``; ``dream.batch(n)`` -> n samples [n,3,H,W] / [n,1,H,W] from one
    ``compose`` call.  The defaults are starting values, NOT tuned on DAVIS."""

    def __init__(self, frame_u8, mask_u8, grow=5, radius=2, passes=3, rots=(-30, 30), scales=(.75, 1.25), fg_shift=0.25, bg_shift=0.05, gain=0.2,
                 offset=20, meanval=MEANVAL, deform=0.0, deform_cell=128, occlude=0.0, band=0):
        from .results import distance_map
        check_lucid(0.0, grow, radius, passes, fg_shift, bg_shift, gain, offset, deform, occlude, band, deform_cell)
        self.deform, self.deform_cell, self.occlude, self.band = float(deform), int(deform_cell), float(occlude), int(band)
        self.ws = None                                                                         # the label plane of the void band, kept between calls
        if not (isinstance(rots, tuple) and isinstance(scales, tuple) and len(rots) == 2 and len(scales) == 2):
            raise ValueError("LucidDream takes continuous (tuple) ranges of rotation and scale")
        if not (-90 <= rots[0] <= rots[1] <= 90 and 0.25 <= scales[0] <= scales[1] <= 4):
            raise ValueError("LucidDream: rots inside -90..90 degrees, scales inside 0.25..4, got %r and %r" % (rots, scales))
        self.frame = _frame(frame_u8, "frame_u8", LUCID_MAX_SIDE)
        self.mask = _plane(mask_u8, self.frame, "mask_u8")
        self.grow, self.radius, self.passes = int(grow), int(radius), int(passes)
        self.rots, self.scales, self.fg_shift, self.bg_shift, self.gain, self.offset = rots, scales, float(fg_shift), float(bg_shift), float(gain), int(offset)
        self.meanval = meanval
        self.h, self.w = int(self.frame.shape[0]), int(self.frame.shape[1])
        self.hole = (distance_map(self.mask)[0] <= self.grow * self.grow).to(torch.uint8)
        self.bg = inpaint(self.frame, self.hole, self.radius, self.passes)
        cols, rows = torch.arange(self.w, device=self.frame.device), torch.arange(self.h, device=self.frame.device)
        on_c, on_r = (self.mask != 0).any(0), (self.mask != 0).any(1)
        box = torch.stack([torch.where(on_c, cols, self.w).min(), torch.where(on_c, cols, -1).max(), torch.where(on_r, rows, self.h).min(),
                           torch.where(on_r, rows, -1).max()]).tolist()                       # the one read-back
        if box[1] < 0:                                                                         # an empty mask
            self.box = None
            self.pivot, self.box_w, self.box_h = (self.w / 2, self.h / 2), 0, 0
        else:
            self.box = tuple(int(v) for v in box)                                              # (x0, x1, y0, y1), inclusive
            self.pivot = ((box[0] + box[1] + 1) / 2, (box[2] + box[3] + 1) / 2)
            self.box_w, self.box_h = box[1] - box[0] + 1, box[3] - box[2] + 1

    def _layer(self):
        rot = (self.rots[1] - self.rots[0]) * random.random() + self.rots[0]
        sc = (self.scales[1] - self.scales[0]) * random.random() + self.scales[0]
        return rot, sc, 2 * random.random() - 1, 2 * random.random() - 1

    def _tone(self):
        g = int(round(256 * (1 + self.gain * (2 * random.random() - 1))))
        o = int(round(self.offset * (2 * random.random() - 1)))
        return [g, g, g, o, o, o]

    def draw(self):
        """-> (matrices [2][6], tones [2][6], field [GH][GW][2] or None, occluder [6] or None) of one sample; the draws in the order of the
        class text"""
        mirror = random.random() < 0.5
        rot, sc, ux, uy = self._layer()
        fg = affine_inverse(self.pivot[0], self.pivot[1], rot, sc, ux * self.fg_shift * self.box_w, uy * self.fg_shift * self.box_h, mirror)
        rot, sc, ux, uy = self._layer()
        bg = affine_inverse(self.w / 2, self.h / 2, rot, sc, ux * self.bg_shift * self.w, uy * self.bg_shift * self.h, mirror)
        tones = [self._tone(), self._tone()]
        field = occ = None
        if self.deform > 0:
            gh, gw = field_shape(self.h, self.w, self.deform_cell)
            amp = 4 * self.deform_cell * self.deform
            field = [[[int(round(amp * (2 * random.random() - 1))) for _ in range(2)] for _ in range(gw)] for _ in range(gh)]
        if self.occlude > 0:
            u = [random.random() for _ in range(7)]
            occ = [0] * 6
            if u[0] < self.occlude and self.box is not None:
                occ = [int(round(self.box[0] + u[1] * self.box_w)), int(round(self.box[2] + u[2] * self.box_h)),
                       int(round((0.1 + 0.2 * u[3]) * self.box_w)), int(round((0.1 + 0.2 * u[4]) * self.box_h)),
                       int(round((2 * u[5] - 1) * self.w / 4)), int(round((2 * u[6] - 1) * self.h / 4))]
        return [fg, bg], tones, field, occ

    def batch(self, n):
        g.check_int("batch", n, 1, LUCID_MAX_BATCH, "lucid")
        draws = [self.draw() for _ in range(n)]
        M, T = [d[0] for d in draws], [d[1] for d in draws]
        if not (self.deform > 0 or self.occlude > 0 or self.band):
            image, gt = compose(self.frame, self.mask, self.bg, M, T, self.meanval)
            return {'image': image, 'gt': gt}
        if self.band and self.ws is None:
            self.ws = g.workspace(lib().osvos_lucid_compose_ex_ws_bytes(LUCID_MAX_BATCH, self.h, self.w, self.band), self.frame.device,
                                  what="%d x %d with band %d" % (self.h, self.w, self.band), prefix="lucid", dtype=torch.int64)
        image, gt = compose(self.frame, self.mask, self.bg, M, T, self.meanval,
                            occluders=[d[3] for d in draws] if self.occlude > 0 else None,
                            field=np.asarray([d[2] for d in draws], np.int16) if self.deform > 0 else None, cell=self.deform_cell,
                            band=self.band, ws=self.ws)
        return {'image': image, 'gt': gt}

    def __call__(self):
        s = self.batch(1)
        return {'image': s['image'][0], 'gt': s['gt'][0]}
