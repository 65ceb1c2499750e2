"""The rule of osvos_lucid_compose_ex (include/osvos_hip.h) restated in numpy -- the composition of tests/lucid_cases.py with a deformation
field on the foreground, an occluder and a void band -- with the naive per-pixel loop and the brute-force band it is checked against, and the
fields, occluders, cases and shared references of tests/test_lucid_deform_cpu.py and tests/test_gpu_lucid_deform.py.  Integers only; every
comparison is np.array_equal.  The references are computed once per process and handed out read-only."""
import functools

import numpy as np

import lucid_cases as lc

MAX_BAND, MIN_CELL, MAX_CELL = 16, 8, 256


def field_shape(h, w, cell):
    s = cell.bit_length() - 1
    assert 1 << s == cell and MIN_CELL <= cell <= MAX_CELL
    return ((h - 1) >> s) + 2, ((w - 1) >> s) + 2


# ---- the rule, vectorised ---------------------------------------------------------------------------------------------------------------

def displacement(D, cell, h, w):
    """(dX, dY) int64 [h,w] of one sample's field D [GH][GW][2] (1/32 pixel): bilinear in the lattice, rounded half up"""
    s = cell.bit_length() - 1
    D = np.asarray(D, np.int64)
    assert D.shape == field_shape(h, w, cell) + (2,)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    gx, gy, tx, ty = xx >> s, yy >> s, xx & (cell - 1), yy & (cell - 1)
    out = []
    for k in (0, 1):
        v = ((cell - tx) * (cell - ty) * D[gy, gx, k] + tx * (cell - ty) * D[gy, gx + 1, k] + (cell - tx) * ty * D[gy + 1, gx, k]
             + tx * ty * D[gy + 1, gx + 1, k] + (1 << (2 * s - 1)))
        assert np.abs(v).max() <= 2 ** 31
        out.append(v >> (2 * s))
    return out[0], out[1]


def covered(occ, h, w):
    """bool [h,w]: inside the ellipse (cx, cy, rx, ry); rx = 0 or ry = 0: nowhere"""
    cx, cy, rx, ry = (int(v) for v in occ[:4])
    if rx == 0 or ry == 0:
        return np.zeros((h, w), bool)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    return (xx - cx) ** 2 * ry * ry + (yy - cy) ** 2 * rx * rx <= rx * rx * ry * ry


def void_band(L, band):
    """bool [h,w]: p is void iff a pixel q inside the image with |p - q|^2 <= band^2 has another label (shifted comparisons)"""
    h, w = L.shape
    out = np.zeros((h, w), bool)
    for dy in range(-band, band + 1):
        for dx in range(-band, band + 1):
            if dy * dy + dx * dx > band * band or (dy == 0 and dx == 0) or abs(dy) >= h or abs(dx) >= w:
                continue
            py, qy = (slice(0, h - dy), slice(dy, h)) if dy >= 0 else (slice(-dy, h), slice(0, h + dy))
            px, qx = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
            out[py, px] |= L[py, px] != L[qy, qx]
    return out


def void_band_brute(L, band):
    """the same, per pixel p a loop over ALL pixels q of the image"""
    h, w = L.shape
    out = np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            out[y, x] = any(L[qy, qx] != L[y, x] and (y - qy) ** 2 + (x - qx) ** 2 <= band * band for qy in range(h) for qx in range(w))
    return out


def compose_ex(bgr, mask, bg, M, tone, occ=None, D=None, cell=64, band=0, mean=lc.MEAN):
    """-> (image float32 [N,3,h,w], gt float32 [N,1,h,w]); gt is -1 where void"""
    h, w = mask.shape
    M, tone = np.asarray(M, np.float64), np.asarray(tone, np.int64)
    n = M.shape[0]
    image, gt = np.empty((n, 3, h, w), np.float32), np.empty((n, 1, h, w), np.float32)
    on = (mask != 0).astype(np.int64)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for i in range(n):
        col = []
        for L, src in ((0, bgr), (1, bg)):
            ix, iy, fx, fy = lc.coordinates(M[i, L], h, w)
            if L == 0 and D is not None:
                dX, dY = displacement(D[i], cell, h, w)
                X, Y = ix * 32 + fx + dX, iy * 32 + fy + dY
                assert max(np.abs(X).max(), np.abs(Y).max()) < 2 ** 31
                ix, iy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
            S = np.zeros((h, w, 3), np.int64)
            a = np.zeros((h, w), np.int64)
            for j in (0, 1):
                for k in (0, 1):
                    wt = (fx if k else 32 - fx) * (fy if j else 32 - fy)
                    ty, tx = iy + j, ix + k
                    cy, cx = np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)
                    S += wt[..., None] * src[cy, cx].astype(np.int64)
                    a += wt * on[cy, cx] * ((ty == cy) & (tx == cx))
            col.append(lc._tone(S, tone[i, L]))
            if L == 0:
                alpha = a
        C = alpha[..., None] * col[0] + (1024 - alpha[..., None]) * col[1]
        label = alpha >= 512
        if occ is not None:
            cov = covered(occ[i], h, w)
            sx, sy = int(occ[i][4]), int(occ[i][5])
            S = 1024 * bg[np.clip(yy + sy, 0, h - 1), np.clip(xx + sx, 0, w - 1)].astype(np.int64)
            C = np.where(cov[..., None], 1024 * lc._tone(S, tone[i, 1]), C)
            label = label & ~cov
        assert C.max() < 2 ** 31 and C.min() >= 0
        image[i] = (C.astype(np.float32) * np.float32(2.0 ** -20) - np.asarray(mean, np.float32)).transpose(2, 0, 1)
        gt[i, 0] = np.where(void_band(label, band), -1.0, label) if band else label
    return image, gt


# ---- the rule, one pixel at a time ------------------------------------------------------------------------------------------------------

def _rn(v):
    return int(np.rint(v))


def compose_ex_naive(bgr, mask, bg, M, tone, occ=None, D=None, cell=64, band=0, mean=lc.MEAN):
    h, w = mask.shape
    n = len(M)
    s = cell.bit_length() - 1
    image, gt = np.empty((n, 3, h, w), np.float32), np.empty((n, 1, h, w), np.float32)
    for i in range(n):
        label = np.zeros((h, w), bool)
        for y in range(h):
            for x in range(w):
                col, alpha = [], 0
                for L, src in ((0, bgr), (1, bg)):
                    m = [float(v) for v in M[i][L]]
                    X = (_rn((m[1] * y + m[2]) * 1024.0) + _rn(m[0] * x * 1024.0) + 16) >> 5
                    Y = (_rn((m[4] * y + m[5]) * 1024.0) + _rn(m[3] * x * 1024.0) + 16) >> 5
                    if L == 0 and D is not None:
                        gx, gy, tx, ty = x >> s, y >> s, x & (cell - 1), y & (cell - 1)
                        d = [[[int(v) for v in D[i][gy + j][gx + k]] for k in (0, 1)] for j in (0, 1)]
                        wts = [[(cell - tx) * (cell - ty), tx * (cell - ty)], [(cell - tx) * ty, tx * ty]]
                        X += (sum(wts[j][k] * d[j][k][0] for j in (0, 1) for k in (0, 1)) + (1 << (2 * s - 1))) >> (2 * s)
                        Y += (sum(wts[j][k] * d[j][k][1] for j in (0, 1) for k in (0, 1)) + (1 << (2 * s - 1))) >> (2 * s)
                    ix, iy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
                    S, a = [0, 0, 0], 0
                    for j in (0, 1):
                        for k in (0, 1):
                            wt = (fx if k else 32 - fx) * (fy if j else 32 - fy)
                            ty_, tx_ = iy + j, ix + k
                            cy, cx = min(max(ty_, 0), h - 1), min(max(tx_, 0), w - 1)
                            for c in range(3):
                                S[c] += wt * int(src[cy, cx, c])
                            if 0 <= ty_ < h and 0 <= tx_ < w and mask[ty_, tx_] != 0:
                                a += wt
                    t = [int(v) for v in tone[i][L]]
                    col.append([min(max(((S[c] * t[c] + 128) >> 8) + t[3 + c] * 1024, 0), 255 << 10) for c in range(3)])
                    if L == 0:
                        alpha = a
                C = [alpha * col[0][c] + (1024 - alpha) * col[1][c] for c in range(3)]
                lab = alpha >= 512
                if occ is not None:
                    cx, cy, rx, ry, sx, sy = (int(v) for v in occ[i])
                    if rx != 0 and ry != 0 and (x - cx) ** 2 * ry ** 2 + (y - cy) ** 2 * rx ** 2 <= rx ** 2 * ry ** 2:
                        t = [int(v) for v in tone[i][1]]
                        px = bg[min(max(y + sy, 0), h - 1), min(max(x + sx, 0), w - 1)]
                        C = [1024 * min(max(((1024 * int(px[c]) * t[c] + 128) >> 8) + t[3 + c] * 1024, 0), 255 << 10) for c in range(3)]
                        lab = False
                for c in range(3):
                    image[i, c, y, x] = np.float32(C[c]) * np.float32(2.0 ** -20) - np.float32(mean[c])
                label[y, x] = lab
        gt[i, 0] = np.where(void_band_brute(label, band), -1.0, label) if band else label
    return image, gt


# ---- fields, occluders, draws -----------------------------------------------------------------------------------------------------------

FIELDS = ("none", "zero", "max", "min", "noise", "smooth")


def field_of(kind, n, h, w, cell):
    """int16 [n][GH][GW][2] or None.  'max' / 'min': every component +32767 / -32768 (1024 pixels: every tap leaves the frame); 'noise':
    +-3 cells, folding freely (the ABI does not care); 'smooth': what LucidDream draws at deform = 1, at most cell / 8 pixels"""
    if kind == "none":
        return None
    gh, gw = field_shape(h, w, cell)
    rng = np.random.default_rng([h, w, cell, n])
    if kind == "zero":
        d = np.zeros((n, gh, gw, 2))
    elif kind == "max":
        d = np.full((n, gh, gw, 2), 32767)
    elif kind == "min":
        d = np.full((n, gh, gw, 2), -32768)
    elif kind == "noise":
        d = rng.integers(-3 * 32 * cell, 3 * 32 * cell + 1, size=(n, gh, gw, 2))
    elif kind == "smooth":
        d = rng.integers(-4 * cell, 4 * cell + 1, size=(n, gh, gw, 2))
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(d.astype(np.int16))


OCCLUDERS = ("none", "inside", "partly_out", "whole", "rx0", "mixed")


def occluders_of(kind, n, h, w):
    """int32 [n][6] (cx, cy, rx, ry, sx, sy) or None"""
    one = {
        "inside": (w // 2, h // 2, max(1, w // 5), max(1, h // 4), 3, -2),
        "partly_out": (-1, h - 1, max(2, w // 3), max(2, h // 2), -w, 2),
        "whole": (w // 2, h // 2, 4096, 4096, 8192, -8192),
        "rx0": (w // 2, h // 2, 0, 5, 1, 1),
        "ry0": (w // 2, h // 2, 5, 0, 1, 1),
        "thin": (w // 3, h // 3, 1, 1, 0, 0),
    }
    if kind == "none":
        return None
    if kind != "mixed":
        return np.asarray([one[kind]] * n, np.int32)
    names = sorted(one)
    return np.asarray([one[names[i % len(names)]] for i in range(n)], np.int32)


def draw(rng_random, box, h, w, deform, deform_cell, occlude):
    """what LucidDream.draw draws AFTER its 13 numbers, written out again: -> (field [GH][GW][2] or None, occluder [6] or None).  box:
    (x0, x1, y0, y1) inclusive, or None for an empty mask"""
    field = occ = None
    if deform > 0:
        gh, gw = field_shape(h, w, deform_cell)
        field = np.zeros((gh, gw, 2), np.int16)
        for gy in range(gh):
            for gx in range(gw):
                for k in (0, 1):
                    field[gy, gx, k] = int(round(4 * deform_cell * deform * (2 * rng_random() - 1)))
    if occlude > 0:
        u = [rng_random() for _ in range(7)]
        occ = [0] * 6
        if u[0] < occlude and box is not None:
            bw, bh = box[1] - box[0] + 1, box[3] - box[2] + 1
            occ = [int(round(box[0] + u[1] * bw)), int(round(box[2] + u[2] * bh)), int(round((0.1 + 0.2 * u[3]) * bw)),
                   int(round((0.1 + 0.2 * u[4]) * bh)), int(round((2 * u[5] - 1) * w / 4)), int(round((2 * u[6] - 1) * h / 4))]
    return field, occ


# ---- cases and shared references --------------------------------------------------------------------------------------------------------

# (h, w, mask kind, parameter set, N, field kind, cell, occluder kind, band).  The composition runs 64 x 4 tiles and a wave's ballot is one
# word of the label plane: 1 x 1; rows of two words with the mask's edge at columns 63 / 64 ('edge64'); three words with a partial last one;
# a lattice the sides are no multiple of (cell 8) and a single lattice cell (cell 64, 256); bands 1, 5, 16 and 16 on a frame 5 rows high
CASES = [(1, 1, "full", "identity", 1, "noise", 8, "inside", 1),
         (1, 1, "empty", "mixed", 3, "zero", 64, "none", 16),
         (5, 70, "edge64", "identity", 1, "none", 64, "none", 1),
         (5, 70, "edge64", "identity", 1, "none", 64, "none", 16),
         (70, 5, "edge64", "mixed", 3, "smooth", 8, "mixed", 5),
         (5, 70, "corner", "mixed", 16, "smooth", 16, "mixed", 16),
         (37, 130, "blob", "mixed", 3, "smooth", 32, "partly_out", 5),
         (37, 130, "checker", "identity", 1, "none", 64, "none", 1),
         (37, 53, "blob", "rot30_s075", 1, "noise", 8, "none", 0),
         (37, 53, "blob", "mixed", 3, "smooth", 64, "inside", 5),
         (37, 53, "blob", "identity", 1, "none", 64, "inside", 0),
         (37, 53, "blob", "identity", 1, "none", 64, "none", 5),
         (37, 53, "blob", "mixed", 3, "noise", 256, "whole", 1),
         (37, 53, "corner", "mixed", 3, "zero", 8, "rx0", 16),
         (37, 53, "blob", "identity", 1, "max", 64, "none", 1),
         (37, 53, "blob", "identity", 1, "min", 64, "none", 1),
         (37, 53, "blob", "shift_part", 1, "min", 256, "none", 0),
         (37, 53, "blob", "mixed", 16, "smooth", 8, "mixed", 5)]
LARGE = (480, 854, "blob", "mixed", 3, "smooth", 128, "mixed", 16)
BATCH = CASES[-1]


def mask_of(kind, h, w):
    if kind == "edge64":                                     # the object ends with column 63: the label edge lies between two words of the plane
        m = np.zeros((h, w), np.uint8)
        m[:, :64] = 255
        return m
    return lc.mask_of(kind, h, w)


def case_id(c):
    return "-".join(str(v) for v in c)


def case_inputs(c):
    h, w, kind, params, n, fkind, cell, okind, band = c
    M, tone = lc.params_of(params, h, w, n)
    return dict(bgr=lc.frame_of("noise", h, w, 2), mask=mask_of(kind, h, w), bg=lc.frame_of("gradient", h, w), M=np.asarray(M, np.float64),
                tone=np.asarray(tone, np.int32), D=field_of(fkind, n, h, w, cell), occ=occluders_of(okind, n, h, w), cell=cell, band=band)


@functools.lru_cache(maxsize=None)
def reference(c):
    r = case_inputs(c)
    r["image"], r["gt"] = compose_ex(r["bgr"], r["mask"], r["bg"], r["M"], r["tone"], r["occ"], r["D"], r["cell"], r["band"])
    return lc._frozen(r)
