"""Appearance matching (csrc/match.hip; the rule: include/osvos_hip.h) restated in numpy, with the case lists, the awkward feature generators and
the two-frame scenario shared by tests/test_match_cpu.py and tests/test_gpu_match.py.

Every float operation is one float32 operation (numpy's float32 multiply, divide and sqrt are correctly rounded); the dot products are formed as
a float64 matmul of the int8 operands, which is exact (|dot| <= 127^2 * 1024 < 2^24).  The device is compared with this bit for bit."""
import functools

import numpy as np

import tta_cases

F32 = np.float32
VOID = 255

# ---------------------------------------------------------------------------------------------------------------- the restatement


def bf16_round(a):
    """float32 -> the float32 value of the nearest bfloat16 (half to even; finite values and infinities)"""
    u = np.ascontiguousarray(a, dtype=F32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7fff + ((u >> 16) & 1)) >> 16 << 16
    return (r & 0xffffffff).astype(np.uint32).view(F32).reshape(np.shape(a))


def quantize(feat):
    """feat float32 [P, C] (a bf16 tensor widened) -> (q int8 [P, C], rinv float32 [P])"""
    f = np.asarray(feat, dtype=F32)
    m = np.abs(f).max(axis=1)                                   # (NaN propagates: not finite)
    dead = ~np.isfinite(f).all(axis=1) | (m == 0)
    with np.errstate(all="ignore"):
        s = np.where(dead, F32(0), F32(127.0) / np.where(dead, F32(1), m)).astype(F32)
        v = np.rint((f * s[:, None]).astype(F32))             # one multiply, half to even
    v = np.where(np.isnan(v), F32(0), v)                        # 0 * inf (s overflowed), and everything of a dead pixel
    v = np.where(dead[:, None], F32(0), v)
    q = np.clip(v, -127, 127).astype(np.int8)
    n = (q.astype(np.int32) ** 2).sum(axis=1, dtype=np.int32)
    with np.errstate(all="ignore"):
        rinv = np.where(n > 0, F32(1.0) / np.sqrt(np.maximum(n, 1).astype(F32)), F32(0)).astype(F32)
    return q, rinv


def grid_shape(h, w, stride):
    return -(-h // stride), -(-w // stride)


def cell_labels(mask, stride):
    """mask uint8 [N, H, W] -> uint8 [N, h, w]: 1 if 4 k >= 3 a, 0 if 4 k <= a, else 255 (a the cell's area inside the frame, k its object pixels)"""
    mask = np.asarray(mask)
    n, H, W = mask.shape
    h, w = grid_shape(H, W, stride)
    obj = np.zeros((n, h * stride, w * stride), np.int64)
    obj[:, :H, :W] = mask != 0
    inside = np.zeros((h * stride, w * stride), np.int64)
    inside[:H, :W] = 1
    k = obj.reshape(n, h, stride, w, stride).sum(axis=(2, 4))
    a = inside.reshape(h, stride, w, stride).sum(axis=(1, 3))[None]
    return np.where(4 * k >= 3 * a, 1, np.where(4 * k <= a, 0, VOID)).astype(np.uint8)


def cell_labels_naive(mask, stride):
    mask = np.asarray(mask)
    n, H, W = mask.shape
    h, w = grid_shape(H, W, stride)
    out = np.zeros((n, h, w), np.uint8)
    for b in range(n):
        for i in range(h):
            for j in range(w):
                cell = mask[b, stride * i:min(stride * i + stride, H), stride * j:min(stride * j + stride, W)]
                a, k = cell.size, int((cell != 0).sum())
                out[b, i, j] = 1 if 4 * k >= 3 * a else (0 if 4 * k <= a else VOID)
    return out


def scores(Q, R, rinv_r):
    """t [Pq, Pr] float32 = (float) dot * rinv_r"""
    dot = Q.astype(np.float64) @ R.astype(np.float64).T        # exact
    assert np.abs(dot).max(initial=0) < 2 ** 24
    return (dot.astype(F32) * np.asarray(rinv_r, F32)[None, :]).astype(F32)


def nearest(Q, rinv_q, R, rinv_r, label_r):
    """Q int8 [N, Pq, C], rinv_q [N, Pq]; R int8 [NR, Pr, C], rinv_r, label_r [NR, Pr] (NR = N or 1)
    -> (sim float32 [N, 2, Pq], idx int32 [N, 2, Pq]); row 0 of the class axis is the foreground (label 1), row 1 the background (label 0)"""
    n, pq, _ = Q.shape
    nr = R.shape[0]
    assert nr in (1, n)
    sim = np.full((n, 2, pq), -2.0, F32)
    idx = np.full((n, 2, pq), -1, np.int32)
    for b in range(n):
        rb = b if nr == n else 0
        t = scores(Q[b], R[rb], rinv_r[rb])
        for row, cls in ((0, 1), (1, 0)):
            cols = np.flatnonzero(label_r[rb] == cls)
            if cols.size == 0:
                continue
            sub = t[:, cols]
            j = sub.argmax(axis=1)                              # the first (smallest b) of the maxima
            idx[b, row] = cols[j]
            sim[b, row] = (sub[np.arange(pq), j] * np.asarray(rinv_q[b], F32)).astype(F32)
    return sim, idx


def nearest_naive(Q, rinv_q, R, rinv_r, label_r):
    """the same with Python loops and integer dots (small cases only)"""
    n, pq, _ = Q.shape
    nr = R.shape[0]
    sim = np.full((n, 2, pq), -2.0, F32)
    idx = np.full((n, 2, pq), -1, np.int32)
    for b in range(n):
        rb = b if nr == n else 0
        for a in range(pq):
            for row, cls in ((0, 1), (1, 0)):
                best, bi = None, -1
                for r in range(R.shape[1]):
                    if label_r[rb, r] != cls:
                        continue
                    t = F32(F32(int(np.dot(Q[b, a].astype(np.int64), R[rb, r].astype(np.int64)))) * F32(rinv_r[rb, r]))
                    if best is None or t > best:
                        best, bi = t, r
                if best is not None:
                    sim[b, row, a] = F32(best * F32(rinv_q[b, a]))
                    idx[b, row, a] = bi
    return sim, idx


def match_map(sim):
    """sim [N, 2, Pq] -> sim_fg - sim_bg, float32 [N, Pq] (one float32 subtraction)"""
    return (sim[:, 0] - sim[:, 1]).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- generators

FEATURE_KINDS = ("relu", "signed", "halves", "extreme")


def features(kind, p, c, seed=0):
    """float32 [p, c] with the awkward pixels planted where p allows: pixel 1 all zero, pixel 2 holds an inf, pixel 3 a NaN, pixel 4 is +-v in every
    channel (q = +-127 everywhere), pixel 6 repeats pixel 5, pixel 7 is tiny (its scale 127 / m overflows)"""
    rng = np.random.default_rng([FEATURE_KINDS.index(kind), p, c, seed])
    if kind == "relu":                                          # post-ReLU-like: sparse, heavy-tailed, non-negative
        f = np.exp(1.5 * rng.standard_normal((p, c))) * (rng.random((p, c)) < 0.3)
    elif kind == "signed":
        f = rng.standard_normal((p, c)) * np.exp(2.0 * rng.standard_normal((p, 1)))
    elif kind == "halves":                                      # m = 127 exactly, so s = 1 and the products are k + 0.5: ties of rint
        f = rng.integers(-253, 254, size=(p, c)) * 0.5
        f[:, 0] = 127.0
    else:                                                       # every channel at the pixel's extreme, random signs
        f = rng.choice([-1.0, 1.0], size=(p, c)) * np.exp(rng.standard_normal((p, 1)))
    f = f.astype(F32)
    if p > 1:
        f[1] = 0
    if p > 2:
        f[2, c // 3] = np.inf
    if p > 3:
        f[3, c - 1] = np.nan
    if p > 4:
        f[4] = np.where(rng.random(c) < 0.5, -3.25, 3.25)
    if p > 6:
        f[6] = f[5]
    if p > 7:
        f[7] = rng.choice(np.array([0, 2e-38, -3e-38], F32), size=c)         # (normal numbers: no subnormal enters the rule's test)
        f[7, 1] = F32(3e-38)
    return f


QUANT_C = (64, 192, 512, 1024)
QUANT_P = (1, 63, 257)
LABEL_CASES = [(48, 64, 8), (45, 70, 8), (37, 53, 4), (9, 9, 16)]                       # (H, W, S)
NEAREST_CASES = [(1, 1, 64), (37, 33, 64), (130, 257, 128), (129, 1000, 512), (300, 2049, 1024)]      # (Pq, Pr, C)
DAVIS_CASE = (6420, 6420, 512)
LABEL_KINDS = ("mixed", "fg", "bg", "void")


def masks(h, w, n, seed=0):
    """uint8 [n, h, w]: blobs with ragged edges, values 0 / 1 / 255 (any nonzero is object)"""
    rng = np.random.default_rng([h, w, n, seed])
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((n, h, w), np.uint8)
    for b in range(n):
        cy, cx = rng.uniform(0.2, 0.8) * h, rng.uniform(0.2, 0.8) * w
        blob = ((yy - cy) / (0.35 * h)) ** 2 + ((xx - cx) / (0.3 * w)) ** 2 < 1
        blob ^= rng.random((h, w)) < 0.05
        blob[-3:, -5:] = True                                   # object reaches into the (ragged) corner cell
        out[b] = np.where(blob, rng.choice([1, 255], size=(h, w)), 0)
    return out


def labels_of(kind, nr, pr, seed=0):
    rng = np.random.default_rng([LABEL_KINDS.index(kind), nr, pr, seed])
    if kind == "fg":
        return np.ones((nr, pr), np.uint8)
    if kind == "bg":
        return np.zeros((nr, pr), np.uint8)
    if kind == "void":
        return rng.choice(np.array([VOID, 2, 7], np.uint8), size=(nr, pr))
    return rng.choice(np.array([1, 0, VOID], np.uint8), size=(nr, pr), p=[0.2, 0.5, 0.3])      # uneven on purpose


@functools.lru_cache(maxsize=None)
def nearest_problem(pq, pr, c, n=2, nr=1, kind="mixed", seed=0):
    """-> dict(Q, rinv_q, R, rinv_r, label, sim, idx): quantised awkward features, asymmetric on purpose (R is not a permutation of Q, the classes
    are uneven), with duplicated reference rows in one tile, in neighbouring tiles and far apart (index ties), query rows that ARE reference rows,
    and, at C = 1024, rows at +-127 everywhere so that |dot| reaches 127^2 C.  The restatement's answer is computed once and is read-only."""
    rng = np.random.default_rng([pq, pr, c, n, nr, LABEL_KINDS.index(kind), seed])
    fq = np.stack([features("relu" if (b + seed) % 2 == 0 else "signed", pq, c, seed + b) for b in range(n)])
    fr = np.stack([features("signed" if (b + seed) % 2 == 0 else "relu", pr, c, seed + 100 + b) for b in range(nr)])
    label = labels_of(kind, nr, pr, seed)
    for b in range(nr):
        for src, dst in ((5, 9), (11, 11 + 128), (20, pr - 1), (0, pr // 2), (130, 131)):      # duplicates: the smaller index must win
            if src < pr and dst < pr and src != dst:
                fr[b, dst] = fr[b, src]
                label[b, dst] = label[b, src]
        if c == 1024 and pr > 40:
            fr[b, 30] = 2.0
            fr[b, 31] = -2.0
            fr[b, 32] = 2.0
            label[b, 30:33] = (1, 0, 1) if kind == "mixed" else label[b, 30:33]
    for b in range(n):
        rb = b if nr == n else 0
        for a in range(8, min(pq, 24)):
            fq[b, a] = fr[rb, (a * 37) % pr]                    # a query identical to a reference row
        if c == 1024 and pq > 40:
            fq[b, 33] = 5.0
            fq[b, 34] = -5.0
    Q, rinv_q = zip(*(quantize(f) for f in fq))
    R, rinv_r = zip(*(quantize(f) for f in fr))
    Q, rinv_q, R, rinv_r = np.stack(Q), np.stack(rinv_q), np.stack(R), np.stack(rinv_r)
    sim, idx = nearest(Q, rinv_q, R, rinv_r, label)
    out = dict(Q=Q, rinv_q=rinv_q, R=R, rinv_r=rinv_r, label=label, sim=sim, idx=idx)
    for v in out.values():
        v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- the scenario

SCENE = dict(H=96, W=128, stride=8, C=64, gain=4.0, noise=0.35, seed=7)
SCENE_IOU_PLAIN = 0.5
SCENE_IOU_MATCHED = 1.0


def iou(a, b):
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    return float((a & b).sum()) / float(max((a | b).sum(), 1))


@functools.lru_cache(maxsize=None)
def scenario():
    """Two frames on an H x W image with a stride-8 feature grid.  Every region has a feature prototype; a cell's feature is its region's prototype
    plus noise, rectified.  Frame 0 is annotated: the object (4 x 4 cells) on background.  In frame 1 the object has moved by (1, 3) cells and a
    distractor (4 x 4 cells) appears whose FEATURES are the background's but whose LOGITS are the object's: the plain mask takes it for the
    object.  -> dict with the features, masks, logits, the restatement's banks, sim, map, the fused logits (float64, tta_cases.fuse_reference)
    and the two IoUs"""
    s = SCENE
    H, W, S, C = s["H"], s["W"], s["stride"], s["C"]
    h, w = grid_shape(H, W, S)
    rng = np.random.default_rng(s["seed"])
    proto = {k: np.maximum(rng.standard_normal(C), 0) * 2.0 for k in ("object", "background")}

    def frame(obj_cell, distractor_cell):
        region = np.zeros((h, w), np.int64)
        region[obj_cell[0]:obj_cell[0] + 4, obj_cell[1]:obj_cell[1] + 4] = 1
        feat = np.where(region[..., None] == 1, proto["object"], proto["background"]) + s["noise"] * rng.standard_normal((h, w, C))
        truth = np.kron(region, np.ones((S, S), np.int64)).astype(np.uint8)
        fires = truth.copy()
        if distractor_cell is not None:
            fires[S * distractor_cell[0]:S * (distractor_cell[0] + 4), S * distractor_cell[1]:S * (distractor_cell[1] + 4)] = 1
        return np.maximum(feat, 0).astype(F32), truth, np.where(fires != 0, F32(2.0), F32(-2.0)).astype(F32)

    f0, mask0, _ = frame((2, 2), None)
    f1, truth1, logits1 = frame((3, 5), (7, 11))
    R, rinv_r = quantize(f0.reshape(h * w, C))
    label = cell_labels(mask0[None], S).reshape(1, h * w)
    Q, rinv_q = quantize(f1.reshape(h * w, C))
    sim, idx = nearest(Q[None], rinv_q[None], R[None], rinv_r[None], label)
    mp = match_map(sim).reshape(1, h, w)
    fused = tta_cases.fuse_reference([logits1[None], mp], [False, False], (H, W), [1.0, s["gain"]])
    out = dict(f0=f0, f1=f1, mask0=mask0, truth1=truth1, logits1=logits1, R=R, rinv_r=rinv_r, label=label, Q=Q, rinv_q=rinv_q, sim=sim, idx=idx, map=mp,
               fused=fused, margin=float(np.abs(fused).min()), iou_plain=iou(logits1 > 0, truth1), iou_matched=iou(fused[0] > 0, truth1), h=h, w=w)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
