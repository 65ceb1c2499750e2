"""TEST INFRASTRUCTURE: the CPU reference of the object-centred zoom kernels (csrc/roi.hip), shared by test_roi_cpu.py and test_gpu_roi.py.
It restates the box rule of include/osvos_hip.h in numpy int64 and builds the two resampling references on tta_cases.resize -- the float64
restatement of the sampling rule -- applied to the cropped array: the view is "the test-time augmentation view of the cropped frame", the
paste is "the map resized to the box, written into an array of ``outside``"."""
import math

import numpy as np

import tta_cases as tc

MEANVAL = tc.MEANVAL
FRAME_SIZES = [(16, 16, 1), (30, 85, 1), (37, 53, 2), (48, 64, 1)]          # (H, W, N): widths off a multiple of 4 and of 16, two frames
CANVASES = [None, (24, 40), (17, 31), (1, 1)]                               # None: the frame's size
MARGINS = [(0, 0), (25, 8), (100, 0)]                                       # (percent, pixels)
ZOOMS = [1, 2, 4]
MASK_NAMES = ["empty", "full", "corner_tl", "corner_tr", "corner_bl", "corner_br", "mid_pixel", "blob_bottom_right", "bar", "two_blobs"]


def min_size(size, canvas, max_zoom):
    """(min_h, min_w) = min(side, ceil(canvas side / max_zoom))"""
    return tuple(min(s, int(math.ceil(c / float(max_zoom)))) for s, c in zip(size, canvas))


def tight(mask):
    """(xa, xb, ya, yb) of the non-zero pixels of a [H,W] array, or None for an empty one"""
    ys, xs = np.nonzero(np.asarray(mask))
    if ys.size == 0:
        return None
    return int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())


def box_rule(mask, canvas, margin_pct, margin_px, min_w, min_h, trace=None):
    """one [H,W] mask -> (x0, y0, bw, bh), every step in numpy int64.  trace: a dict that receives 'clamped' (step 5 changed the box)"""
    i64 = np.int64
    h, w = (i64(v) for v in np.asarray(mask).shape)
    hc, wc = i64(canvas[0]), i64(canvas[1])
    t = tight(mask)
    if t is None:
        if trace is not None:
            trace["clamped"] = False
        return 0, 0, int(w), int(h)
    xa, xb, ya, yb = (i64(v) for v in t)
    bw, bh = xb - xa + 1, yb - ya + 1
    pad = (max(bw, bh) * i64(margin_pct) + 99) // 100 + i64(margin_px)
    x0, y0 = xa - pad, ya - pad
    bw, bh = bw + 2 * pad, bh + 2 * pad
    if bw < min_w:
        x0, bw = x0 - (i64(min_w) - bw) // 2, i64(min_w)
    if bh < min_h:
        y0, bh = y0 - (i64(min_h) - bh) // 2, i64(min_h)
    if bw * hc < bh * wc:
        nw = (bh * wc + hc - 1) // hc
        x0, bw = x0 - (nw - bw) // 2, nw
    elif bh * wc < bw * hc:
        nh = (bw * hc + wc - 1) // wc
        y0, bh = y0 - (nh - bh) // 2, nh
    before = (x0, y0, bw, bh)
    bw, bh = min(bw, w), min(bh, h)
    x0, y0 = min(max(x0, i64(0)), w - bw), min(max(y0, i64(0)), h - bh)
    if trace is not None:
        trace["clamped"] = before != (x0, y0, bw, bh)
    return int(x0), int(y0), int(bw), int(bh)


def boxes(masks, canvas, margin_pct, margin_px, max_zoom):
    """[N,H,W] masks -> int32 [N,4], with the minimum size the Python layer derives from max_zoom"""
    masks = np.asarray(masks)
    min_h, min_w = min_size(masks.shape[1:], canvas, max_zoom)
    return np.array([box_rule(m, canvas, margin_pct, margin_px, min_w, min_h) for m in masks], dtype=np.int32).reshape(-1, 4)


def view_reference(frames_u8, box, canvas, meanval=MEANVAL):
    """uint8 [N,H,W,3], boxes [N,4] -> float64 [N,3,Hc,Wc]: tta_cases.view_reference of each frame's crop"""
    out = []
    for f, (x0, y0, bw, bh) in zip(np.asarray(frames_u8), np.asarray(box)):
        out.append(tc.view_reference(f[None, y0:y0 + bh, x0:x0 + bw], canvas[0], canvas[1], meanval=meanval)[0])
    return np.stack(out)


def paste_reference(logits, box, size, outside):
    """[N,Hc,Wc] maps, boxes [N,4] -> (float64 [N,H,W], bool [N,H,W] inside the box)"""
    h, w = size
    out = np.full((len(logits), h, w), np.float64(np.float32(outside)))
    inside = np.zeros((len(logits), h, w), dtype=bool)
    for n, (x0, y0, bw, bh) in enumerate(np.asarray(box)):
        out[n, y0:y0 + bh, x0:x0 + bw] = tc.resize(logits[n], bh, bw)
        inside[n, y0:y0 + bh, x0:x0 + bw] = True
    return out, inside


def named_mask(name, h, w):
    """uint8 [h,w] -- the named cases of the issue"""
    m = np.zeros((h, w), dtype=np.uint8)
    if name == "empty":
        pass
    elif name == "full":
        m[:] = 1
    elif name == "corner_tl":
        m[0, 0] = 1
    elif name == "corner_tr":
        m[0, w - 1] = 255
    elif name == "corner_bl":
        m[h - 1, 0] = 1
    elif name == "corner_br":
        m[h - 1, w - 1] = 7
    elif name == "mid_pixel":
        m[h // 2, w // 2] = 1
    elif name == "blob_bottom_right":
        m[h - max(2, h // 4):, w - max(3, w // 5):] = 1
    elif name == "bar":                      # 3 pixels wide, full height: the aspect growth overshoots W and clamps
        m[:, w // 3:w // 3 + 3] = 1
    elif name == "two_blobs":
        m[1:1 + max(1, h // 8), 2:2 + max(1, w // 8)] = 1
        m[h - 2 - max(1, h // 8):h - 2, w - 3 - max(1, w // 8):w - 3] = 1
    else:
        raise KeyError(name)
    return m


def random_mask(h, w, seed):
    """a seeded mask: a few rectangles and single pixels, sometimes none"""
    rng = np.random.default_rng(4000 + seed)
    m = np.zeros((h, w), dtype=np.uint8)
    for _ in range(int(rng.integers(0, 4))):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        m[y:y + int(rng.integers(1, max(2, h // 2))), x:x + int(rng.integers(1, max(2, w // 2)))] = 1
    for _ in range(int(rng.integers(0, 3))):
        m[int(rng.integers(0, h)), int(rng.integers(0, w))] = 1
    return m


def mask_batches(h, w, n):
    """[(name, uint8 [n,h,w])]: every named mask on frame 0; further frames take the next names, so a batch of two always holds two
    different boxes, and ('empty+blob') an empty mask and a non-empty one in the same call"""
    out = []
    for i, name in enumerate(MASK_NAMES):
        out.append((name, np.stack([named_mask(MASK_NAMES[(i + 3 * k) % len(MASK_NAMES)], h, w) for k in range(n)])))
    if n >= 2:
        out.append(("empty+blob", np.stack([named_mask("empty", h, w), named_mask("blob_bottom_right", h, w)] + [named_mask("full", h, w)] * (n - 2))))
    return out
