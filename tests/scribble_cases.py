"""Restatements and cases shared by tests/test_scribble_cpu.py and tests/test_gpu_scribble.py (osvos_pytorch_amd.scribble: the stroke raster
and the Guo-Hall skeleton of include/osvos_hip.h, "interactive scribbles").

``raster_bruteforce`` evaluates the coverage rule with Python integers, pixel by pixel and segment by segment; ``raster_ref`` is the same rule
in int64 numpy over whole frames (the CPU tests hold it against the brute force, the GPU tests use it).  ``thin_ref`` is the thinning rule on a
zero-padded boolean plane.  ``components8`` labels 8-connected components by tests/component_cases.py's canonical rule -- a component's label
is 1 + the lowest flat index of its pixels, the largest is the one of the largest area and the lowest label on a tie -- and
``initial_ref`` / ``error_ref`` restate the simulated annotator on top of these.  Nothing here imports the code under test.
"""
import numpy as np

UNLABELLED = 255
LIST_CAP = 512          # OSVOS_SCRIBBLE_LIST_CAP: rows of a tile's LDS list; RASTER_CASES["many"] puts 700 over one tile, two passes
CHUNK = 256             # rows culled at a time


def covers_int(px, py, seg, r):
    """the coverage rule with Python integers"""
    x0, y0, x1, y1 = (int(v) for v in seg[:4])
    dx, dy, wx, wy = x1 - x0, y1 - y0, px - x0, py - y0
    L, t = dx * dx + dy * dy, wx * dx + wy * dy
    if L == 0 or t <= 0:
        return wx * wx + wy * wy <= r * r
    if t >= L:
        return (px - x1) ** 2 + (py - y1) ** 2 <= r * r
    return (wx * dy - wy * dx) ** 2 <= r * r * L


def raster_bruteforce(segs, n, h, w, r):
    out = np.full((n, h, w), UNLABELLED, dtype=np.uint8)
    for f in range(n):
        for y in range(h):
            for x in range(w):
                for s in segs:          # ascending: the last covering row stays
                    if int(s[5]) == f and covers_int(x, y, s, r):
                        out[f, y, x] = int(s[4])
    return out


def raster_ref(segs, n, h, w, r):
    """int64 numpy: the same bytes as ``raster_bruteforce`` (coordinates below 2^14: nothing overflows)"""
    out = np.full((n, h, w), UNLABELLED, dtype=np.uint8)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    r2 = np.int64(r) * r
    for s in np.asarray(segs, dtype=np.int64).reshape(-1, 6):
        x0, y0, x1, y1, value, f = s
        if not 0 <= f < n:
            continue
        dx, dy, wx, wy = x1 - x0, y1 - y0, xx - x0, yy - y0
        L, t = dx * dx + dy * dy, wx * dx + wy * dy
        near_a = wx * wx + wy * wy <= r2
        near_b = (xx - x1) ** 2 + (yy - y1) ** 2 <= r2
        cross = wx * dy - wy * dx
        cov = np.where((L == 0) | (t <= 0), near_a, np.where(t >= L, near_b, cross * cross <= r2 * L))
        out[f][cov] = value
    return out


def _table(rows):
    return np.asarray(rows, dtype=np.int32).reshape(-1, 6)


def raster_cases():
    """name -> (segs int32 [M,6], (N, H, W)); every case is rastered at each of RADII"""
    rng = np.random.RandomState(5)
    cases = {}
    cases["none"] = (_table([]), (1, 33, 70))
    cases["pixel"] = (_table([(0, 0, 0, 0, 1, 0)]), (1, 1, 1))
    cases["point"] = (_table([(40, 17, 40, 17, 3, 0)]), (1, 33, 70))
    # horizontal, vertical and both diagonals across the 64-column and 16-row tile edges; endpoints beyond W and H
    cases["lines"] = (_table([(2, 15, 69, 16, 1, 0), (63, 0, 64, 32, 2, 0), (0, 0, 69, 32, 0, 0), (69, 1, 3, 30, 4, 0), (50, 20, 500, 300, 5, 0),
                              (10, 40, 30, 90, 6, 0), (16383, 16383, 60, 30, 7, 0)]), (1, 33, 70))
    a, b = (5, 5, 60, 28, 1, 0), (5, 28, 60, 5, 2, 0)
    cases["overlap_ab"] = (_table([a, b]), (1, 33, 70))
    cases["overlap_ba"] = (_table([b, a]), (1, 33, 70))
    rows = []
    for i in range(40):                  # three frames interleaved, padding rows (frame -1) in between
        f = (-1, 0, 1, 2)[i % 4]
        rows.append(tuple(rng.randint(0, 48, size=4)) + (int(rng.randint(0, 5)), f))
    cases["frames"] = (_table(rows), (3, 40, 40))
    # 700 short segments, all over the tile at columns 0..63 and rows 0..15: three cull chunks of 256 and, with a list of 512 rows, two passes
    rows = [(int(rng.randint(0, 64)), int(rng.randint(0, 16)), int(rng.randint(0, 64)), int(rng.randint(0, 16)), int(rng.randint(0, 255)), 0)
            for _ in range(700)]
    cases["many"] = (_table(rows), (1, 33, 70))
    return cases


RADII = (0, 1, 3, 64)


# ---- thinning --------------------------------------------------------------------------------------------------------------------------

def thin_substep(m, sub):
    """one sub-step on a boolean plane [H,W] -> the plane afterwards"""
    p = np.pad(m, 1)
    P2, P3, P4, P5 = p[:-2, 1:-1], p[:-2, 2:], p[1:-1, 2:], p[2:, 2:]
    P6, P7, P8, P9 = p[2:, 1:-1], p[2:, :-2], p[1:-1, :-2], p[:-2, :-2]
    i = lambda a: a.astype(np.int32)
    C = i(~P2 & (P3 | P4)) + i(~P4 & (P5 | P6)) + i(~P6 & (P7 | P8)) + i(~P8 & (P9 | P2))
    N1 = i(P9 | P2) + i(P3 | P4) + i(P5 | P6) + i(P7 | P8)
    N2 = i(P2 | P3) + i(P4 | P5) + i(P6 | P7) + i(P8 | P9)
    Nm = np.minimum(N1, N2)
    side = ((P2 | P3 | ~P5) & P4) if sub == 0 else ((P6 | P7 | ~P9) & P8)
    return m & ~((C == 1) & (Nm >= 2) & (Nm <= 3) & ~side)


def thin_ref(mask, max_iters=64):
    """mask [N,H,W] (non-zero = set) -> (skeleton uint8 [N,H,W], info int32 [N,2]: iterations run, 1 if the last deleted nothing)"""
    mask = np.asarray(mask) != 0
    out, info = np.zeros(mask.shape, dtype=np.uint8), np.zeros((mask.shape[0], 2), dtype=np.int32)
    for n, m in enumerate(mask):
        iters, still = 0, 0
        while iters < max_iters:
            nxt = thin_substep(thin_substep(m, 0), 1)
            iters += 1
            if (nxt == m).all():
                still = 1
                break
            m = nxt
        out[n], info[n] = m, (iters, still)
    return out, info


def components8(mask):
    """bool [H,W] -> int32 labels: 0 off the mask, else 1 + the lowest flat index of the pixel's 8-connected component"""
    h, w = mask.shape
    lab = np.zeros((h, w), dtype=np.int32)
    for y0 in range(h):
        for x0 in range(w):
            if mask[y0, x0] and lab[y0, x0] == 0:
                root, stack = 1 + y0 * w + x0, [(y0, x0)]
                lab[y0, x0] = root
                while stack:
                    y, x = stack.pop()
                    for yy in range(max(y - 1, 0), min(y + 2, h)):
                        for xx in range(max(x - 1, 0), min(x + 2, w)):
                            if mask[yy, xx] and lab[yy, xx] == 0:
                                lab[yy, xx] = root
                                stack.append((yy, xx))
    return lab


def count8(mask):
    lab = components8(np.asarray(mask) != 0)
    return len(np.unique(lab[lab > 0]))


def kept_components(mask, min_area=0, keep_largest=False):
    """the selection rule without a seed: at least min_area pixels, and with keep_largest the largest (the lowest label on a tie)"""
    lab = components8(mask)
    ids, areas = np.unique(lab[lab > 0], return_counts=True)
    keep = np.zeros(mask.shape, dtype=bool)
    if ids.size == 0:
        return keep
    largest = ids[np.argmax(areas)]          # (argmax: the first of equal areas, ids ascending)
    for i, a in zip(ids, areas):
        if a >= min_area and (not keep_largest or i == largest):
            keep |= lab == i
    return keep


def sqdist_to(mask):
    """exact squared distance of every pixel to the nearest set pixel; a huge number in a frame without one"""
    h, w = mask.shape
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return np.full((h, w), 2 ** 31 - 1, dtype=np.int64)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return ((yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2).min(axis=-1)


def stroke_ref(region, radius, max_iters=64):
    s = thin_ref(region[None], max_iters)[0][0] != 0
    return region & (sqdist_to(s) <= radius * radius)


def initial_ref(gt, radius=3, max_iters=64):
    out = np.full(gt.shape, UNLABELLED, dtype=np.uint8)
    for n in range(gt.shape[0]):
        for v in np.unique(gt):
            if v == UNLABELLED:
                continue
            region = kept_components(gt[n] == v, keep_largest=True)
            out[n][stroke_ref(region, radius, max_iters)] = v
    return out


def error_ref(pred, gt, min_area=64, keep_largest=True, radius=3, max_iters=64):
    out = np.full(gt.shape, UNLABELLED, dtype=np.uint8)
    for n in range(gt.shape[0]):
        kept = kept_components(pred[n] != gt[n], min_area, keep_largest)
        s = stroke_ref(kept, radius, max_iters)
        out[n][s] = gt[n][s]
    return out


def blob(h, w, seed, fill=0.5):
    """a random smooth-ish boolean blob plane"""
    rng = np.random.RandomState(seed)
    a = rng.rand(h + 4, w + 4)
    a = sum(a[dy:dy + h, dx:dx + w] for dy in range(5) for dx in range(5)) / 25.0
    return a > np.quantile(a, 1.0 - fill)


def thin_cases():
    """name -> uint8 [N,H,W] masks (non-zero = set; some set bytes are not 1)"""
    cases = {}
    cases["pixel"] = np.ones((1, 1, 1), dtype=np.uint8)
    m = np.zeros((1, 5, 64), dtype=np.uint8); m[0, 1:4, 3:61] = 7
    cases["bar64"] = m
    m = np.zeros((1, 7, 65), dtype=np.uint8); m[0, 1:6, 58:65] = 1; m[0, 3, 0:58] = 255
    cases["across63"] = m
    m = np.zeros((2, 9, 128), dtype=np.uint8); m[0, 2:8, 60:70] = 1; m[0, 0:9, 120:128] = 1; m[1, 4, :] = 1; m[1, :, 64] = 1
    cases["across_words"] = m
    m = np.zeros((1, 40, 130), dtype=np.uint8); m[0, 5:30, 120:130] = 1; m[0, 10:20, 60:68] = 1; m[0, 33:39, 125:130] = 1
    cases["across127"] = m
    cases["full"] = np.ones((1, 40, 130), dtype=np.uint8)
    m = np.zeros((1, 40, 130), dtype=np.uint8)
    for i in range(40):
        m[0, i, i] = 1; m[0, i, 129 - i] = 1; m[0, i, 60 + i] = 1
    cases["diagonals"] = m
    yy, xx = np.meshgrid(np.arange(9), np.arange(128), indexing="ij")
    cases["checkerboard"] = np.stack([((yy + xx) % 2 == 0), ((yy + xx) % 2 == 1)]).astype(np.uint8)
    m = np.zeros((1, 44, 130), dtype=np.uint8); m[0, 2:42, 45:85] = 1
    cases["square40"] = m          # roughly 20 iterations
    m = np.zeros((3, 40, 130), dtype=np.uint8); m[0, 18:22, 10:120] = 1; m[1, 2:38, 40:100] = 1; m[2, 20, 5] = 1
    cases["batch3"] = m            # three frames that converge after different numbers of iterations
    cases["blobs"] = np.stack([blob(40, 130, 1), blob(40, 130, 2, 0.3)]).astype(np.uint8)
    m = np.zeros((1, 4, 4), dtype=np.uint8); m[0, 1:3, 1:3] = 1
    cases["square2"] = m
    return cases


WIDE = (3, 33, 16000)      # 33 rows of 250 words = 8250 words: more than the 8000 path 1 keeps in LDS


def wide_case():
    m = np.zeros(WIDE, dtype=np.uint8)
    m[0, 3:30, 100:15900] = 1
    m[1, 10:14, 63:129] = 1; m[1, 0:33, 8000:8006] = 1
    m[2] = np.tile(blob(33, 500, 3), (1, 32))
    return m
