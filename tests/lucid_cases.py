"""The lucid rules of include/osvos_hip.h (osvos_lucid_inpaint, osvos_lucid_compose) restated in numpy, with the naive per-pixel loops they
are checked against, and the scenes, masks, parameter sets and shared references of tests/test_lucid_cpu.py and tests/test_gpu_lucid.py.
Integers only (int64 here; the limits keep everything inside int32 on the device): every comparison is np.array_equal.  The references are
computed once per process and handed out read-only."""
import functools
import math

import numpy as np

MEAN = (104.00699, 116.66877, 122.67892)
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
NEUTRAL = (256, 256, 256, 0, 0, 0)
DEFAULTS = dict(grow=5, radius=2, passes=3)


# ---- scenes and masks -------------------------------------------------------------------------------------------------------------------

def frame_of(kind, h, w, seed=0):
    """uint8 [h,w,3]: 'noise' (every pixel its own colour, so that a wrong arg-min shows) or 'gradient'"""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if kind == "noise":
        return np.random.default_rng([h, w, seed]).integers(0, 256, size=(h, w, 3)).astype(np.uint8)
    if kind == "gradient":
        return np.stack([(xx * 3 + yy) % 256, (yy * 5 + 40) % 256, (xx + 2 * yy + 90) % 256], -1).astype(np.uint8)
    raise KeyError(kind)


MASKS = ("empty", "full", "corner", "ring", "sides", "checker", "blob", "dots")


def mask_of(kind, h, w):
    """uint8 [h,w] with values 0 / 255 (and a few 1: any non-zero byte counts).  As a HOLE: 'ring' leaves a one-pixel non-hole frame around
    a filled rectangle; 'sides' leaves exactly one non-hole pixel in the middle of each side, at equal distance from the centre when the
    sides are odd and equal; 'dots' leaves a sparse lattice of non-hole pixels (many exact ties)."""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if kind == "empty":
        m = np.zeros((h, w), bool)
    elif kind == "full":
        m = np.ones((h, w), bool)
    elif kind == "corner":                                   # touches the top and the left border
        m = (yy < max(1, (2 * h) // 3)) & (xx < max(1, w // 2))
    elif kind == "ring":
        m = (yy >= 1) & (yy < h - 1) & (xx >= 1) & (xx < w - 1)
    elif kind == "sides":
        m = np.ones((h, w), bool)
        for y, x in ((0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1)):
            m[y, x] = False
    elif kind == "checker":
        m = (yy + xx) % 2 == 0
    elif kind == "blob":
        m = ((yy - 0.45 * h) / (0.28 * h + 0.5)) ** 2 + ((xx - 0.55 * w) / (0.2 * w + 0.5)) ** 2 <= 1
    elif kind == "dots":
        m = ~((yy % 4 == 1) & (xx % 6 == 2))
    else:
        raise KeyError(kind)
    out = m.astype(np.uint8) * 255
    out[m & ((yy * 7 + xx) % 5 == 0)] = 1
    return out


def sqdist(mask):
    """int64 [h,w]: the exact squared distance to the nearest set pixel, 2^31 - 1 without one (brute force; small frames only)"""
    h, w = mask.shape
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return np.full((h, w), 2 ** 31 - 1, np.int64)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return ((yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2).min(-1)


def grow_hole(mask, grow):
    return (sqdist(mask) <= grow * grow).astype(np.uint8)


# ---- inpainting -------------------------------------------------------------------------------------------------------------------------

def column_nearest(hole):
    """int64 [h,w]: the row of the nearest non-hole pixel of the same column, the smaller row on a tie, -1 in a column without one"""
    h, w = hole.shape
    rows = np.arange(h)[:, None]
    free = hole == 0
    up = np.maximum.accumulate(np.where(free, rows, -1), axis=0)
    dn = np.minimum.accumulate(np.where(free, rows, 2 * h + 8)[::-1], axis=0)[::-1]
    take_up = (up >= 0) & ((dn > h) | (rows - up <= dn - rows))
    return np.where(take_up, up, np.where(dn > h, -1, dn))


def fill(bgr, hole):
    """the two-pass fill: the column answers, then per row and hole pixel the minimiser of (d, qy, qx) over the columns' candidates"""
    h, w = hole.shape
    near = column_nearest(hole)
    out = bgr.copy()
    cols = np.arange(w)
    for y in range(h):
        hx = np.nonzero(hole[y])[0]
        c = near[y]
        ok = np.nonzero(c >= 0)[0]
        if hx.size == 0 or ok.size == 0:
            continue
        key = (((hx[:, None] - ok[None, :]) ** 2 + (c[ok] - y)[None, :] ** 2) << 24) + (c[ok][None, :] << 12) + cols[ok][None, :]
        q = ok[np.argmin(key, axis=1)]
        out[y, hx] = bgr[c[q], q]
    return out


def fill_brute(bgr, hole):
    """per hole pixel, a search over every non-hole pixel of the frame for the smallest (|p - q|^2, qy, qx)"""
    h, w = hole.shape
    out = bgr.copy()
    free = [(y, x) for y in range(h) for x in range(w) if hole[y, x] == 0]
    if not free:
        return out
    for y in range(h):
        for x in range(w):
            if hole[y, x]:
                _, qy, qx = min(((y - fy) ** 2 + (x - fx) ** 2, fy, fx) for fy, fx in free)
                out[y, x] = bgr[qy, qx]
    return out


def smooth(img, hole, radius, passes):
    h, w = hole.shape
    y0, y1 = np.maximum(np.arange(h) - radius, 0), np.minimum(np.arange(h) + radius, h - 1) + 1
    x0, x1 = np.maximum(np.arange(w) - radius, 0), np.minimum(np.arange(w) + radius, w - 1) + 1
    n = ((y1 - y0)[:, None] * (x1 - x0)[None, :])[..., None]
    cur = img.copy()
    for _ in range(passes):
        ii = np.zeros((h + 1, w + 1, 3), np.int64)
        ii[1:, 1:] = cur.astype(np.int64).cumsum(0).cumsum(1)
        s = ii[y1][:, x1] - ii[y0][:, x1] - ii[y1][:, x0] + ii[y0][:, x0]
        cur = np.where((hole != 0)[..., None], (2 * s + n) // (2 * n), cur).astype(np.uint8)
    return cur


def smooth_naive(img, hole, radius, passes):
    h, w = hole.shape
    cur = img.copy()
    for _ in range(passes):
        nxt = cur.copy()
        for y in range(h):
            for x in range(w):
                if hole[y, x]:
                    win = cur[max(y - radius, 0):y + radius + 1, max(x - radius, 0):x + radius + 1].reshape(-1, 3).astype(int)
                    n = win.shape[0]
                    for c in range(3):
                        nxt[y, x, c] = (2 * int(win[:, c].sum()) + n) // (2 * n)
        cur = nxt
    return cur


def inpaint(bgr, hole, radius=2, passes=3):
    return smooth(fill(bgr, hole), hole, radius, passes)


# ---- composition ------------------------------------------------------------------------------------------------------------------------

def coordinates(M, h, w):
    """(ix, iy, fx, fy) int64 [h,w] of one dst -> src affine, formed as osvos_augment_frame forms them"""
    M = [float(v) for v in M]
    x, y = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)
    adelta, bdelta = np.rint(M[0] * x * 1024.0).astype(np.int64), np.rint(M[3] * x * 1024.0).astype(np.int64)
    xb, yb = np.rint((M[1] * y + M[2]) * 1024.0).astype(np.int64), np.rint((M[4] * y + M[5]) * 1024.0).astype(np.int64)
    X, Y = (xb[:, None] + adelta[None, :] + 16) >> 5, (yb[:, None] + bdelta[None, :] + 16) >> 5
    return X >> 5, Y >> 5, X & 31, Y & 31


def _tone(S, t):
    g, o = np.asarray(t[:3], np.int64), np.asarray(t[3:], np.int64)
    return np.clip(((S * g + 128) >> 8) + o * 1024, 0, 255 << 10)


def compose(bgr, mask, bg, M, tone, mean=MEAN):
    """-> (image float32 [N,3,h,w], gt float32 [N,1,h,w])"""
    h, w = mask.shape
    M, tone = np.asarray(M, np.float64), np.asarray(tone, np.int64)
    n = M.shape[0]
    image, gt = np.empty((n, 3, h, w), np.float32), np.empty((n, 1, h, w), np.float32)
    on = (mask != 0).astype(np.int64)
    for i in range(n):
        col = []
        for L, src in ((0, bgr), (1, bg)):
            ix, iy, fx, fy = coordinates(M[i, L], h, w)
            S = np.zeros((h, w, 3), np.int64)
            a = np.zeros((h, w), np.int64)
            for j in (0, 1):
                for k in (0, 1):
                    wt = (fx if k else 32 - fx) * (fy if j else 32 - fy)
                    ty, tx = iy + j, ix + k
                    cy, cx = np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)
                    S += wt[..., None] * src[cy, cx].astype(np.int64)
                    a += wt * on[cy, cx] * ((ty == cy) & (tx == cx))
            col.append(_tone(S, tone[i, L]))
            if L == 0:
                alpha = a
        C = alpha[..., None] * col[0] + (1024 - alpha[..., None]) * col[1]
        assert C.max() < 2 ** 31 and C.min() >= 0
        image[i] = (C.astype(np.float32) * np.float32(2.0 ** -20) - np.asarray(mean, np.float32)).transpose(2, 0, 1)
        gt[i, 0] = alpha >= 512
    return image, gt


def _rn(v):
    return int(np.rint(v))


def compose_naive(bgr, mask, bg, M, tone, mean=MEAN):
    h, w = mask.shape
    n = len(M)
    image, gt = np.empty((n, 3, h, w), np.float32), np.empty((n, 1, h, w), np.float32)
    for i in range(n):
        for y in range(h):
            for x in range(w):
                col, alpha = [], 0
                for L, src in ((0, bgr), (1, bg)):
                    m = [float(v) for v in M[i][L]]
                    X = (_rn((m[1] * y + m[2]) * 1024.0) + _rn(m[0] * x * 1024.0) + 16) >> 5
                    Y = (_rn((m[4] * y + m[5]) * 1024.0) + _rn(m[3] * x * 1024.0) + 16) >> 5
                    ix, iy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
                    S, a = [0, 0, 0], 0
                    for j in (0, 1):
                        for k in (0, 1):
                            wt = (fx if k else 32 - fx) * (fy if j else 32 - fy)
                            ty, tx = iy + j, ix + k
                            cy, cx = min(max(ty, 0), h - 1), min(max(tx, 0), w - 1)
                            for c in range(3):
                                S[c] += wt * int(src[cy, cx, c])
                            if 0 <= ty < h and 0 <= tx < w and mask[ty, tx] != 0:
                                a += wt
                    t = [int(v) for v in tone[i][L]]
                    col.append([min(max(((S[c] * t[c] + 128) >> 8) + t[3 + c] * 1024, 0), 255 << 10) for c in range(3)])
                    if L == 0:
                        alpha = a
                for c in range(3):
                    C = alpha * col[0][c] + (1024 - alpha) * col[1][c]
                    image[i, c, y, x] = np.float32(C) * np.float32(2.0 ** -20) - np.float32(mean[c])
                gt[i, 0, y, x] = 1.0 if alpha >= 512 else 0.0
    return image, gt


def affine_inverse(cx, cy, rot=0.0, sc=1.0, dx=0.0, dy=0.0, mirror=False):
    """what osvos_pytorch_amd.lucid.affine_inverse documents, written out again"""
    a = rot * math.pi / 180.0
    c, s = math.cos(a) / sc, math.sin(a) / sc
    m0, m1, m3, m4 = (-c, s, s, c) if mirror else (c, -s, s, c)
    tx, ty = cx + dx, cy + dy
    return [v + 0.0 for v in (m0, m1, cx - m0 * tx - m1 * ty, m3, m4, cy - m3 * tx - m4 * ty)]


PARAMS = ("identity", "shift_part", "shift_out", "rot30_s075", "rotm30_s125", "mirror", "tone_low", "tone_high", "mixed")


def params_of(kind, h, w, n):
    """(M [n][2][6], tone [n][2][6]) of a named parameter set; 'mixed' walks through all the others and seeded random ones, a different
    set for every sample"""
    cx, cy = w / 2, h / 2
    one = {
        "identity": ([IDENTITY, IDENTITY], [NEUTRAL, NEUTRAL]),
        "shift_part": ([affine_inverse(cx, cy, dx=-(w // 2) - 1, dy=h // 3), affine_inverse(cx, cy, dx=2, dy=-1)], [NEUTRAL, NEUTRAL]),
        "shift_out": ([affine_inverse(cx, cy, dx=w + 1, dy=0), IDENTITY], [NEUTRAL, NEUTRAL]),
        "rot30_s075": ([affine_inverse(cx, cy, 30.0, 0.75, 1.5, -2.25), affine_inverse(cx, cy, -30.0, 0.75)], [NEUTRAL, NEUTRAL]),
        "rotm30_s125": ([affine_inverse(cx * 0.8, cy * 1.1, -30.0, 1.25), affine_inverse(cx, cy, 30.0, 1.25, -3.0, 0.5)], [NEUTRAL, NEUTRAL]),
        "mirror": ([affine_inverse(cx, cy, 7.0, 1.0, 0.0, 0.0, True), affine_inverse(cx, cy, mirror=True)], [NEUTRAL, NEUTRAL]),
        "tone_low": ([IDENTITY, affine_inverse(cx, cy, 3.0)], [(0, 40, 256, -255, -200, -255), (1, 0, 128, -3, 0, -255)]),
        "tone_high": ([affine_inverse(cx, cy, -4.0, 1.1), IDENTITY], [(1024, 1024, 700, 255, 0, 255), (1024, 300, 256, 255, 255, 100)]),
    }
    if kind != "mixed":
        return [one[kind][0]] * n, [one[kind][1]] * n
    rng = np.random.default_rng([h, w, n])
    names = sorted(one)
    M, tone = [], []
    for i in range(n):
        if i % 2 == 0:
            m, t = one[names[(i // 2) % len(names)]]
        else:
            m = [affine_inverse(cx + rng.uniform(-3, 3), cy + rng.uniform(-3, 3), rng.uniform(-30, 30), rng.uniform(0.75, 1.25),
                                rng.uniform(-0.4, 0.4) * w, rng.uniform(-0.4, 0.4) * h, bool(rng.integers(2))) for _ in range(2)]
            t = [tuple(int(v) for v in rng.integers(150, 400, 3)) + tuple(int(v) for v in rng.integers(-40, 41, 3)) for _ in range(2)]
        M.append(m)
        tone.append(t)
    return M, tone


# ---- cases and shared references ------------------------------------------------------------------------------------------------------

# (h, w, mask kind as the HOLE, radius, passes).  The row pass runs 256 lanes per row, the column pass 64 per workgroup, the smoothing 64 x 4
# tiles: 1 x 1; narrower than a wave / shorter than a tile both ways; odd sides; one past each tile edge; and (LARGE) one DAVIS-sized frame
INPAINT_CASES = [(1, 1, "empty", 1, 1), (1, 1, "full", 2, 3), (5, 70, "corner", 2, 3), (70, 5, "checker", 1, 2), (37, 53, "blob", 2, 3),
                 (37, 53, "full", 3, 2), (37, 53, "empty", 2, 1), (9, 9, "ring", 1, 0), (9, 9, "sides", 8, 1), (11, 11, "sides", 2, 0),
                 (5, 257, "sides", 2, 8), (65, 65, "dots", 3, 1), (12, 15, "ring", 2, 2), (37, 53, "corner", 8, 4)]
INPAINT_LARGE = (480, 854, "blob", 2, 3)

# (h, w, mask kind as the OBJECT, parameter set, N).  The composition runs 64 x 4 tiles
COMPOSE_CASES = [(1, 1, "full", "identity", 1), (1, 1, "empty", "mixed", 3), (5, 70, "corner", "mixed", 16), (70, 5, "checker", "mixed", 3),
                 (37, 53, "blob", "identity", 1), (37, 53, "blob", "shift_part", 1), (37, 53, "blob", "shift_out", 1),
                 (37, 53, "corner", "rot30_s075", 1), (37, 53, "blob", "rotm30_s125", 3), (37, 53, "blob", "mirror", 1),
                 (37, 53, "full", "tone_low", 1), (37, 53, "checker", "tone_high", 1), (5, 65, "blob", "mixed", 16), (37, 53, "empty", "mixed", 16)]
COMPOSE_LARGE = (480, 854, "blob", "mixed", 3)


def case_id(c):
    return "-".join(str(v) for v in c)


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def inpaint_reference(c):
    h, w, kind, radius, passes = c
    bgr, hole = frame_of("noise", h, w, 1), mask_of(kind, h, w)
    filled = fill(bgr, hole)
    return _frozen(dict(bgr=bgr, hole=hole, filled=filled, out=smooth(filled, hole, radius, passes)))


@functools.lru_cache(maxsize=None)
def compose_reference(c):
    h, w, kind, params, n = c
    bgr, mask = frame_of("noise", h, w, 2), mask_of(kind, h, w)
    bg = frame_of("gradient", h, w)
    M, tone = params_of(params, h, w, n)
    image, gt = compose(bgr, mask, bg, M, tone)
    return _frozen(dict(bgr=bgr, mask=mask, bg=bg, M=np.asarray(M, np.float64), tone=np.asarray(tone, np.int32), image=image, gt=gt))


# ---- the scenario: a textured square on a gradient background, moved by one object width ------------------------------------------------

SCENE = dict(h=40, w=64, y0=14, x0=12, side=12)


def scenario_scene():
    """(frame uint8 [h,w,3], mask uint8 [h,w], the background alone uint8 [h,w,3]).  Background: a slow blue-green gradient (R <= 52);
    object: a red two-colour texture (R >= 200)"""
    s = SCENE
    yy, xx = np.meshgrid(np.arange(s["h"]), np.arange(s["w"]), indexing="ij")
    back = np.stack([120 + xx, 100 + yy, 20 + (xx + yy) // 4], -1).astype(np.uint8)
    tex = np.where((((yy // 3) + (xx // 3)) % 2 == 0)[..., None], (30, 40, 240), (60, 20, 200)).astype(np.uint8)
    mask = np.zeros((s["h"], s["w"]), np.uint8)
    mask[s["y0"]:s["y0"] + s["side"], s["x0"]:s["x0"] + s["side"]] = 255
    return np.where(mask[..., None] != 0, tex, back), mask, back


@functools.lru_cache(maxsize=None)
def scenario_reference():
    """the composites of the scenario with the object moved right by its own width: over the frame itself (no inpainting) and over the
    inpainted frame (hole = the mask grown by DEFAULTS['grow'])"""
    s = SCENE
    frame, mask, back = scenario_scene()
    hole = grow_hole(mask, DEFAULTS["grow"])
    bg = inpaint(frame, hole, DEFAULTS["radius"], DEFAULTS["passes"])
    M = [[affine_inverse(0.0, 0.0, dx=s["side"]), IDENTITY]]
    tone = [[NEUTRAL, NEUTRAL]]
    zero = (0.0, 0.0, 0.0)
    plain, gt = compose(frame, mask, frame, M, tone, zero)
    lucid, gt2 = compose(frame, mask, bg, M, tone, zero)
    assert np.array_equal(gt, gt2)
    return _frozen(dict(frame=frame, mask=mask, back=back, hole=hole, bg=bg, M=np.asarray(M), tone=np.asarray(tone, np.int32), plain=plain[0],
                        lucid=lucid[0], gt=gt[0, 0]))
