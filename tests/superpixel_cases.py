"""Numpy restatement of the superpixel rules of include/osvos_hip.h (grid-SLIC on the decoded uint8 BGR frame, and logit pooling over a
labelling), the cases the CPU and the GPU tests share, seeded scenes and the snapping scenario.  Everything is integer arithmetic: the tests
compare with np.array_equal.

The restatement follows the rule literally, not the kernels: `assign` visits the nine cells around a pixel's home cell in ascending cluster
index with a strict `<` (so the smaller k wins a tie), `update` is a per-label integer sum and one floor division, and the pooled logit is
the floor-divided mean of the quantised logits.  Distances are taken in int64 so that the 32-bit claim of the header can be checked.
"""
import numpy as np

# (H, W, N, cell, compactness, iters)
SLIC_CASES = [
    (1, 1, 1, 2, 0, 1),
    (7, 9, 1, 4, 10, 3),
    (37, 53, 2, 8, 10, 5),
    (16, 300, 1, 2, 64, 2),              # more than one tile across, the smallest cell
    (70, 70, 1, 64, 1, 2),               # the largest cell, a 2 x 2 grid
    (33, 65, 1, 5, 0, 4),                # colour only
    (40, 64, 3, 8, 10, 0),               # no iteration: the grid
]
LARGE_CASE = (480, 854, 1, 8, 10, 5)
LARGE_SCENES = ("noise", "two_colour")
SCENES = ("noise", "gradient", "constant", "two_colour")
DEFAULTS = dict(cell=8, compactness=10, iters=5)
Q_ONE = 65536                            # the pooled logits are means of rint(clamp(x, -Q_CLAMP, Q_CLAMP) * Q_ONE)
Q_CLAMP = 16384.0


def case_id(c):
    return "%dx%dx%d_S%d_m%d_T%d" % tuple(c)


def grid_shape(h, w, cell):
    return -(-h // cell), -(-w // cell)


# ---- SLIC -----------------------------------------------------------------------------------------------------------------------------

def home_labels(h, w, cell):
    """int32 [H,W]: the cluster of every pixel's home cell"""
    gw = grid_shape(h, w, cell)[1]
    return ((np.arange(h) // cell)[:, None] * gw + (np.arange(w) // cell)[None, :]).astype(np.int32)


def update(frame, labels, prev, k):
    """frame uint8 [H,W,3], labels int [H,W], prev int [K,6] or None -> centres int64 [K,6] = (x, y, b, g, r, count): per component
    floor((2 sum + count) / (2 count)) over the pixels that carry the label; a cluster without pixels keeps prev (count 0)"""
    h, w = labels.shape
    lab = labels.ravel().astype(np.int64)
    comp = np.concatenate([np.broadcast_to(np.arange(w)[None, :, None], (h, w, 1)), np.broadcast_to(np.arange(h)[:, None, None], (h, w, 1)),
                           frame.astype(np.int64)], axis=-1).reshape(-1, 5).astype(np.int64)
    sums = np.zeros((k, 5), np.int64)
    np.add.at(sums, lab, comp)
    count = np.bincount(lab, minlength=k).astype(np.int64)
    out = np.zeros((k, 6), np.int64)
    full = count > 0
    out[full, :5] = (2 * sums[full] + count[full, None]) // (2 * count[full, None])
    if not full.all():
        out[~full, :5] = prev[~full, :5]
    out[:, 5] = count
    return out


def distances(frame, centres, cell, compactness):
    """-> (D int64 [9,H,W], k int64 [9,H,W], valid bool [9,H,W]) of the nine candidates of every pixel, in ascending k"""
    h, w = frame.shape[:2]
    gh, gw = grid_shape(h, w, cell)
    gy, gx = (np.arange(h) // cell)[:, None], (np.arange(w) // cell)[None, :]
    yy, xx = np.arange(h)[:, None], np.arange(w)[None, :]
    px = frame.astype(np.int64)
    ds_, ks, valid = [], [], []
    for oy in (-1, 0, 1):
        for ox in (-1, 0, 1):
            cy, cx = gy + oy, gx + ox
            ok = (cy >= 0) & (cy < gh) & (cx >= 0) & (cx < gw)
            k = np.clip(cy, 0, gh - 1) * gw + np.clip(cx, 0, gw - 1)
            c = centres[k]                                                   # [H,W,6]
            dc = ((px - c[..., 2:5]) ** 2).sum(-1)
            ds = (xx - c[..., 0]) ** 2 + (yy - c[..., 1]) ** 2
            ds_.append(cell * cell * dc + compactness * compactness * ds)
            ks.append(np.broadcast_to(k, (h, w)))
            valid.append(np.broadcast_to(ok, (h, w)))
    return np.stack(ds_), np.stack(ks), np.stack(valid)


def assign(frame, centres, cell, compactness):
    """int32 [H,W]: per pixel the minimiser of (D, k) over the clusters of the 3 x 3 cells around its home cell that lie in the grid"""
    d, k, ok = distances(frame, centres, cell, compactness)
    best = np.full(d.shape[1:], np.iinfo(np.int64).max)
    lab = np.zeros(d.shape[1:], np.int64)
    for i in range(9):
        better = ok[i] & (d[i] < best)
        best = np.where(better, d[i], best)
        lab = np.where(better, k[i], lab)
    return lab.astype(np.int32)


def slic_one(frame, cell, compactness, iters):
    h, w = frame.shape[:2]
    gh, gw = grid_shape(h, w, cell)
    labels = home_labels(h, w, cell)
    centres = update(frame, labels, None, gh * gw)
    for _ in range(iters):
        labels = assign(frame, centres, cell, compactness)
        centres = update(frame, labels, centres, gh * gw)
    return labels, centres.astype(np.int32)


def slic(frames, cell=8, compactness=10, iters=5):
    """uint8 [N,H,W,3] -> (labels int32 [N,H,W], centres int32 [N,K,6])"""
    out = [slic_one(f, cell, compactness, iters) for f in frames]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def slic_naive(frames, cell, compactness, iters):
    """the rule as loops over pixels and candidates (tiny frames only)"""
    n, h, w = frames.shape[:3]
    gh, gw = grid_shape(h, w, cell)
    k_all = gh * gw
    labels = np.zeros((n, h, w), np.int32)
    centres = np.zeros((n, k_all, 6), np.int32)
    for f in range(n):
        lab = [[(y // cell) * gw + x // cell for x in range(w)] for y in range(h)]
        cen = [None] * k_all
        for t in range(iters + 1):
            if t:
                new = [[0] * w for _ in range(h)]
                for y in range(h):
                    for x in range(w):
                        best = None
                        for cy in range(y // cell - 1, y // cell + 2):
                            for cx in range(x // cell - 1, x // cell + 2):
                                if not (0 <= cy < gh and 0 <= cx < gw):
                                    continue
                                k = cy * gw + cx
                                c = cen[k]
                                dc = sum((int(frames[f, y, x, i]) - c[2 + i]) ** 2 for i in range(3))
                                ds = (x - c[0]) ** 2 + (y - c[1]) ** 2
                                key = (cell * cell * dc + compactness * compactness * ds, k)
                                if best is None or key < best:
                                    best = key
                        new[y][x] = best[1]
                lab = new
            sums = [[0] * 6 for _ in range(k_all)]
            for y in range(h):
                for x in range(w):
                    s = sums[lab[y][x]]
                    for i, v in enumerate((x, y) + tuple(int(v) for v in frames[f, y, x])):
                        s[i] += v
                    s[5] += 1
            cen = [([(2 * s[i] + s[5]) // (2 * s[5]) for i in range(5)] if s[5] else list(cen[k][:5])) + [s[5]] for k, s in enumerate(sums)]
        labels[f], centres[f] = np.array(lab), np.array(cen)
    return labels, centres


# ---- pooling --------------------------------------------------------------------------------------------------------------------------

def quantise(x):
    """float32 [...] -> int64: rint(clamp(x, -Q_CLAMP, Q_CLAMP) * Q_ONE), half to even; NaN -> the lower clamp"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(x), np.float32(-Q_CLAMP), np.clip(x, np.float32(-Q_CLAMP), np.float32(Q_CLAMP))).astype(np.float32)
    return np.rint(c * np.float32(Q_ONE)).astype(np.int64)


def pool(logits, labels, k):
    """float32 [N,H,W], int [N,H,W], K -> float32 [N,H,W]: per label the floor-divided mean of the quantised logits, times 2^-16; a pixel
    whose label is outside [0, K) keeps its logit bit for bit and contributes to nothing"""
    logits = np.asarray(logits, np.float32)
    out = logits.copy()
    for n in range(logits.shape[0]):
        lab = labels[n].astype(np.int64)
        inside = (lab >= 0) & (lab < k)
        q = quantise(logits[n])
        sums = np.zeros(k, np.int64)
        np.add.at(sums, lab[inside], q[inside])
        count = np.bincount(lab[inside], minlength=k).astype(np.int64)
        mean = np.zeros(k, np.int64)
        full = count > 0
        mean[full] = (2 * sums[full] + count[full]) // (2 * count[full])     # (numpy's // is floor division)
        res = mean.astype(np.float32) * np.float32(1.0 / Q_ONE)
        out[n][inside] = res[lab[inside]]
    return out


def pool_naive(logits, labels, k):
    out = np.array(logits, np.float32)
    for n in range(out.shape[0]):
        sums, count = [0] * k, [0] * k
        for l, v in zip(labels[n].ravel().tolist(), logits[n].ravel()):
            if 0 <= l < k:
                sums[l] += int(quantise(v))
                count[l] += 1
        flat = out[n].reshape(-1)
        for i, l in enumerate(labels[n].ravel().tolist()):
            if 0 <= l < k:
                flat[i] = np.float32((2 * sums[l] + count[l]) // (2 * count[l])) * np.float32(1.0 / Q_ONE)
    return out


def awkward_logits(shape, seed):
    """float32 logits with NaN, +-inf, values beyond the clamp, halves of the quantisation step and ordinary values"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 6).astype(np.float32)
    flat = x.reshape(-1)
    special = np.array([np.nan, np.inf, -np.inf, 3e4, -3e4, 16384.0, -16384.0, 0.5 / Q_ONE, 1.5 / Q_ONE, -0.5 / Q_ONE, -2.5 / Q_ONE, 1e-30, -0.0],
                       np.float32)
    at = rng.permutation(flat.size)[:min(flat.size, 4 * special.size)]
    flat[at] = special[np.arange(at.size) % special.size]
    return x


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------

def frames_of(kind, h, w, n, seed=0):
    """uint8 [N,H,W,3].  'noise': independent bytes; 'gradient': a smooth ramp, many near-ties; 'constant': one colour, every distance
    ties and the (D, k) order decides; 'two_colour': two flat colours either side of a slanted line, which empties the clusters it cuts"""
    rng = np.random.default_rng([seed, h, w, n, SCENES.index(kind)])
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if kind == "noise":
        return rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    if kind == "constant":
        f = np.empty((n, h, w, 3), np.uint8)
        f[...] = rng.integers(0, 256, size=(n, 1, 1, 3), dtype=np.uint8)
        return f
    if kind == "gradient":
        f = np.stack([(3 * xx + 2 * yy + 7 * i) // 4 % 256 for i in range(n)], 0)
        return np.stack([f, (f * 2 + yy[None]) % 256, 255 - f], axis=-1).astype(np.uint8)
    if kind == "two_colour":
        side = (3 * xx + 2 * yy) * 2 >= 3 * w + 2 * h
        pal = rng.integers(0, 96, size=(n, 2, 3))
        pal[:, 1] += 140
        return np.where(side[None, :, :, None], pal[:, None, None, 1], pal[:, None, None, 0]).astype(np.uint8)
    raise ValueError(kind)


_cache = {}


def reference(kind, c):
    """-> dict(frames, labels, centres) of scene `kind` under case c; computed once per process, never modified"""
    key = (kind,) + tuple(c)
    if key not in _cache:
        h, w, n, cell, compactness, iters = c
        frames = frames_of(kind, h, w, n)
        labels, centres = slic(frames, cell, compactness, iters)
        for a in (frames, labels, centres):
            a.setflags(write=False)
        _cache[key] = dict(frames=frames, labels=labels, centres=centres)
    return _cache[key]


# ---- the snapping scenario ------------------------------------------------------------------------------------------------------------

SNAP = dict(h=61, w=83, cell=6, compactness=6, iters=3, obj=(40, 90, 200), back=(120, 130, 60), noise=12, shift=2, sigma=3.0, scale=4.0,
            logit_noise=1.5, seed=1)


def _blur(a, sigma):
    r = int(3 * sigma + 0.5)
    g = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    g /= g.sum()
    p = np.pad(a, r, mode="edge")
    p = sum(g[i] * p[i:i + a.shape[0]] for i in range(2 * r + 1))
    return sum(g[i] * p[:, i:i + a.shape[1]] for i in range(2 * r + 1))


def snapping_scene():
    """-> (frame uint8 [H,W,3], truth bool [H,W], logits float32 [H,W]): a filled ellipse on a flat background under uniform colour noise,
    and the logits of a network that sees it two pixels off and blurred: the truth shifted, Gaussian-blurred, scaled, plus noise"""
    s = SNAP
    h, w = s["h"], s["w"]
    rng = np.random.default_rng(s["seed"])
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    truth = ((xx - 0.5 * w) / (0.3 * w)) ** 2 + ((yy - 0.5 * h) / (0.32 * h)) ** 2 <= 1.0
    frame = np.where(truth[..., None], np.array(s["obj"]), np.array(s["back"])) + rng.integers(-s["noise"], s["noise"] + 1, size=(h, w, 3))
    frame = np.clip(frame, 0, 255).astype(np.uint8)
    moved = np.roll(truth, (s["shift"], s["shift"]), axis=(0, 1))
    soft = _blur(moved.astype(np.float64), s["sigma"])
    logits = (s["scale"] * (2 * soft - 1) + rng.normal(0, s["logit_noise"], size=(h, w))).astype(np.float32)
    return frame, truth, logits


def iou(a, b):
    return float((a & b).sum()) / float((a | b).sum())


def snapping_reference():
    """-> dict(frame, truth, logits, labels, k, pooled, iou_plain, iou_pooled, impure) on the restatement; computed once"""
    if "snap" not in _cache:
        s = SNAP
        frame, truth, logits = snapping_scene()
        labels, _ = slic(frame[None], s["cell"], s["compactness"], s["iters"])
        gh, gw = grid_shape(s["h"], s["w"], s["cell"])
        pooled = pool(logits[None], labels, gh * gw)[0]
        inside = np.bincount(labels[0][truth], minlength=gh * gw)
        outside = np.bincount(labels[0][~truth], minlength=gh * gw)
        for a in (frame, truth, logits, labels, pooled):
            a.setflags(write=False)
        _cache["snap"] = dict(frame=frame, truth=truth, logits=logits, labels=labels[0], k=gh * gw, pooled=pooled,
                              iou_plain=iou(logits > 0, truth), iou_pooled=iou(pooled > 0, truth),
                              impure=int(np.minimum(inside, outside).sum()))
    return _cache["snap"]
