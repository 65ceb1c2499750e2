"""numpy restatements for the online-adaptation tests -- no device code: the exact squared Euclidean distance map by brute force (column
distances, then a broadcast minimum per row), the adaptation targets made from two of them (include/osvos_hip.h, "online adaptation"),
and the case lists the CPU and GPU tests share."""
import numpy as np

NONE = 2147483647                       # OSVOS_SQDIST_NONE
POS_LOGIT = float(np.log(0.97 / 0.03))  # what adaptation_targets(prob=0.97) hands the library (rounded to float32 on the way in)

SQDIST_SIZES = [(2, 37, 65), (1, 5, 1030), (1, 64, 257), (3, 1, 63), (1, 33, 1), (1, 2, 64)]
MASK_KINDS = ["empty", "full", "corners", "p0.002", "p0.5", "stripes7", "middle_empty"]


def column_distance(src):
    """src: bool [H,W] -> int64 [H,W]: |y - y'| to the nearest source pixel of the same column, -1 in a column without one"""
    h, w = src.shape
    yy = np.arange(h, dtype=np.int64)
    dy = np.abs(yy[:, None] - yy[None, :])                                   # [y, y']
    big = np.int64(1) << 40
    g = np.where(src[None, :, :], dy[:, :, None], big).min(axis=1)           # [y, x]
    return np.where(g >= big, np.int64(-1), g)


def sqdist_reference(src):
    """src: bool [N,H,W] (True = source pixel) -> int32 [N,H,W]: min over the sources q of the same image of |p - q|^2, NONE without one"""
    src = np.asarray(src, dtype=bool)
    n, h, w = src.shape
    xx = np.arange(w, dtype=np.int64)
    dx2 = (xx[:, None] - xx[None, :]) ** 2                                   # [x, x']
    big = np.int64(1) << 40
    out = np.empty((n, h, w), dtype=np.int64)
    for k in range(n):
        g = column_distance(src[k])
        for y in range(h):
            col = np.where(g[y] >= 0, g[y] ** 2, big)
            out[k, y] = (dx2 + col[None, :]).min(axis=1)
    return np.where(out >= big, np.int64(NONE), out).astype(np.int32)


def sqdist_of_mask(mask, invert):
    """the library's source rule on a uint8 mask: (mask != 0) != invert"""
    return sqdist_reference((np.asarray(mask) != 0) != bool(invert))


def eroded(prev_mask, erosion):
    """E = { p in prev_mask : sqdist(p, background) > erosion^2 }; without a background pixel nothing is eroded"""
    m = np.asarray(prev_mask) != 0
    d = sqdist_reference(~m).astype(np.int64)
    return m & ((d == NONE) | (d > int(erosion) ** 2))


def targets_reference(logits, prev_mask, pos_logit, erosion, distance):
    """logits float32 [N,H,W], prev_mask [N,H,W] -> (label float32 [N,H,W] of 1 / 0 / -1, counts int64 [N,3] = n_pos, n_neg, n_void)"""
    logits = np.asarray(logits, dtype=np.float32)
    d = sqdist_reference(eroded(prev_mask, erosion)).astype(np.int64)
    neg = (d == NONE) | (d > int(distance) ** 2)
    with np.errstate(invalid="ignore"):
        pos = ~neg & (logits > np.float32(pos_logit))
    label = np.where(neg, np.float32(0), np.where(pos, np.float32(1), np.float32(-1))).astype(np.float32)
    n = label.shape[0]
    counts = np.stack([pos.reshape(n, -1).sum(1), neg.reshape(n, -1).sum(1), (~pos & ~neg).reshape(n, -1).sum(1)], axis=1).astype(np.int64)
    return label, counts


def make_mask(kind, n, h, w, seed=0):
    """uint8 [N,H,W] (set pixels are 255, or odd non-zero bytes where that can matter)"""
    rng = np.random.RandomState(1000 + seed)
    m = np.zeros((n, h, w), dtype=np.uint8)
    if kind == "empty":
        pass
    elif kind == "full":
        m[:] = 1
    elif kind == "corners":
        m[:, 0, 0] = m[:, 0, w - 1] = m[:, h - 1, 0] = m[:, h - 1, w - 1] = 255
    elif kind == "p0.002":
        m[rng.rand(n, h, w) < 0.002] = 255
    elif kind == "p0.5":
        m[rng.rand(n, h, w) < 0.5] = 7
    elif kind == "stripes7":
        m[:, :, ::7] = (rng.rand(n, h, len(range(0, w, 7))) < 0.3) * 255
        m[:, :, 3::7] = 0
    elif kind == "middle_empty":
        m[rng.rand(n, h, w) < 0.01] = 255
        m[n // 2] = 0
        if n == 1:
            m[0, :, : w // 2] = 0
    else:
        raise ValueError(kind)
    return m


def ellipse(h, w, cx=0.5, cy=0.5, ry=0.25, rx=0.2):
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    return (((yy - cy * h) / (ry * h)) ** 2 + ((xx - cx * w) / (rx * w)) ** 2) <= 1


# (H, W, erosion, distance, (n_pos, n_neg, n_void)) on target_case's inputs at POS_LOGIT.  n_neg is geometry alone (2479, 1449, 3967); n_pos and
# n_void follow the noise of target_case's generator.  All three classes are non-empty in every case.
TARGET_CASES = [(48, 80, 2, 9, (380, 2479, 981)), (37, 53, 0, 3, (185, 1449, 327)), (64, 96, 3, 12, (604, 3967, 1573))]


def target_case(h, w, seed=0):
    """prev_mask uint8 [1,H,W]: the ellipse moved right by 5 % of the width; logits float32 [1,H,W]: +4 inside the centred ellipse, -4
    outside, plus 1.5 sigma of Gaussian noise"""
    prev = ellipse(h, w, cx=0.55)
    now = ellipse(h, w)
    rng = np.random.RandomState(seed)
    logits = np.where(now, 4.0, -4.0) + 1.5 * rng.randn(h, w)
    return logits.astype(np.float32)[None], (prev.astype(np.uint8) * 255)[None]
