"""Top-K averaging and the local window of appearance matching (csrc/match_ext.hip; the rules: include/osvos_hip.h) restated in numpy on top of
tests/match_cases.py, with the case lists and two scenarios built like match_cases.scenario(), shared by tests/test_match_ext_cpu.py and
tests/test_gpu_match_ext.py.

As in match_cases every float operation is one float32 operation and the dot products are exact; the device is compared bit for bit."""
import functools

import numpy as np

import match_cases as mc
import tta_cases

F32 = np.float32
MAX_K, MAX_RADIUS = 16, 15

# ---------------------------------------------------------------------------------------------------------------- the restatement


def topk(Q, rinv_q, R, rinv_r, label_r, K):
    """the operands of match_cases.nearest -> sim float32 [N, 2, Pq]: per class the k = min(K, rows of the class) largest scores, summed from the
    largest down in float32, divided by (float) k, times rinv_q; -2 for an empty class"""
    assert 1 <= K <= MAX_K
    n, pq, _ = Q.shape
    nr = R.shape[0]
    assert nr in (1, n)
    sim = np.full((n, 2, pq), -2.0, F32)
    for b in range(n):
        rb = b if nr == n else 0
        t = mc.scores(Q[b], R[rb], rinv_r[rb])
        for row, cls in ((0, 1), (1, 0)):
            cols = np.flatnonzero(label_r[rb] == cls)
            if cols.size == 0:
                continue
            k = min(K, cols.size)
            best = -np.sort(-t[:, cols], axis=1)[:, :k]         # descending (negation is exact; the rule's operands give no -0)
            s = best[:, 0].copy()
            for i in range(1, k):
                s = (s + best[:, i]).astype(F32)
            sim[b, row] = ((s / F32(k)).astype(F32) * np.asarray(rinv_q[b], F32)).astype(F32)
    return sim


def _score(q, r, rinv):
    return F32(F32(int(np.dot(q.astype(np.int64), r.astype(np.int64)))) * F32(rinv))


def topk_naive(Q, rinv_q, R, rinv_r, label_r, K):
    """the same with Python loops and integer dots (small cases only)"""
    n, pq, _ = Q.shape
    nr = R.shape[0]
    sim = np.full((n, 2, pq), -2.0, F32)
    for b in range(n):
        rb = b if nr == n else 0
        for a in range(pq):
            for row, cls in ((0, 1), (1, 0)):
                ts = sorted((_score(Q[b, a], R[rb, r], rinv_r[rb, r]) for r in range(R.shape[1]) if label_r[rb, r] == cls), reverse=True)[:K]
                if not ts:
                    continue
                s = ts[0]
                for v in ts[1:]:
                    s = F32(s + v)
                sim[b, row, a] = F32(F32(s / F32(len(ts))) * F32(rinv_q[b, a]))
    return sim


def local(Q, rinv_q, R, rinv_r, label_r, h, w, radius):
    """Q and R on the same h x w grid (P = h w rows each, row-major) -> (sim float32 [N, 2, P], idx int32 [N, 2, P]): nearest over the reference
    cells within `radius` rows and columns of the query cell; the smallest row of the maxima; (-2, -1) when the window holds no row of the class"""
    assert 0 <= radius <= MAX_RADIUS
    n, p, _ = Q.shape
    nr = R.shape[0]
    assert p == h * w and R.shape[1] == p and nr in (1, n)
    ii, jj = np.divmod(np.arange(p), w)
    window = (np.abs(ii[:, None] - ii[None, :]) <= radius) & (np.abs(jj[:, None] - jj[None, :]) <= radius)
    sim = np.full((n, 2, p), -2.0, F32)
    idx = np.full((n, 2, p), -1, np.int32)
    for b in range(n):
        rb = b if nr == n else 0
        t = mc.scores(Q[b], R[rb], rinv_r[rb])
        for row, cls in ((0, 1), (1, 0)):
            cand = window & (label_r[rb] == cls)[None, :]
            tt = np.where(cand, t, F32(-np.inf))                # (every score is finite)
            j = tt.argmax(axis=1)                               # the first (smallest row) of the maxima
            has = cand.any(axis=1)
            with np.errstate(invalid="ignore"):                 # (-inf * 0 in a window without the class: replaced below)
                best = (tt[np.arange(p), j] * np.asarray(rinv_q[b], F32)).astype(F32)
            sim[b, row] = np.where(has, best, F32(-2.0))
            idx[b, row] = np.where(has, j, -1)
    return sim, idx


def local_naive(Q, rinv_q, R, rinv_r, label_r, h, w, radius):
    n, p, _ = Q.shape
    nr = R.shape[0]
    sim = np.full((n, 2, p), -2.0, F32)
    idx = np.full((n, 2, p), -1, np.int32)
    for b in range(n):
        rb = b if nr == n else 0
        for i in range(h):
            for j in range(w):
                a = i * w + j
                for row, cls in ((0, 1), (1, 0)):
                    best, bi = None, -1
                    for y in range(max(i - radius, 0), min(i + radius, h - 1) + 1):
                        for x in range(max(j - radius, 0), min(j + radius, w - 1) + 1):
                            r = y * w + x
                            if label_r[rb, r] != cls:
                                continue
                            t = _score(Q[b, a], R[rb, r], rinv_r[rb, r])
                            if best is None or t > best:
                                best, bi = t, r
                    if best is not None:
                        sim[b, row, a] = F32(best * F32(rinv_q[b, a]))
                        idx[b, row, a] = bi
    return sim, idx


def local_map(sim):
    """sim [N, 2, P] -> max(sim_fg, -1) - max(sim_bg, -1), float32 [N, P]: three float32 operations; an empty class is the smallest cosine"""
    return (np.maximum(sim[:, 0], F32(-1.0)) - np.maximum(sim[:, 1], F32(-1.0))).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- the cases

# (Pq, Pr, C, K): one row; fewer rows than K in a class and one slice; across the 128-row query and reference tiles; several slices;
# rows at +-127 everywhere
TOPK_CASES = [(1, 1, 64, 1), (37, 33, 64, 4), (130, 257, 128, 3), (129, 1000, 512, 8), (300, 2049, 1024, 16)]
TOPK_DAVIS_CASE = (6420, 6420, 512, 4)
# (h, w, C, radius): one cell; a small ragged grid; a window that covers the grid (= nearest); several 4 x 8 tiles, ragged; a wide grid, many
# channels; the most channels (16 pieces per lane, rows at +-127 everywhere)
LOCAL_CASES = [(1, 1, 64, 0), (5, 7, 64, 2), (9, 13, 128, 15), (33, 41, 64, 3), (12, 67, 512, 4), (6, 7, 1024, 2)]
LOCAL_DAVIS_CASE = (60, 107, 512, 4)


@functools.lru_cache(maxsize=None)
def topk_problem(pq, pr, c, k, n=2, nr=1, kind="mixed"):
    """match_cases.nearest_problem's operands (duplicated rows, queries that are reference rows, +-127 rows) with the restatement's top-K sim,
    computed once and read-only"""
    p = dict(mc.nearest_problem(pq, pr, c, n=n, nr=nr, kind=kind))
    p["topk"] = topk(p["Q"], p["rinv_q"], p["R"], p["rinv_r"], p["label"], k)
    p["topk"].setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def local_problem(h, w, c, radius, n=2, nr=1, kind="mixed"):
    """match_cases.nearest_problem's operands at Pq = Pr = h w with the restatement's local (sim, idx), computed once and read-only"""
    p = dict(mc.nearest_problem(h * w, h * w, c, n=n, nr=nr, kind=kind))
    p["lsim"], p["lidx"] = local(p["Q"], p["rinv_q"], p["R"], p["rinv_r"], p["label"], h, w, radius)
    p["lsim"].setflags(write=False)
    p["lidx"].setflags(write=False)
    return p


# ---------------------------------------------------------------------------------------------------------------- the scenarios

BLEED = dict(H=96, W=128, stride=8, C=64, gain=6.0, noise=0.35, seed=7, cell=(6, 3), K=4)
BLEED_IOU_PLAIN = 0.5
BLEED_IOU_K1 = 0.5
BLEED_IOU_K4 = 1.0
TWIN = dict(H=96, W=128, stride=8, C=64, gain=4.0, local_gain=6.0, radius=5, noise=0.35, seed=7, twin=(7, 11))
TWIN_IOU_PLAIN = 0.5
TWIN_IOU_FIRST = 0.5
TWIN_IOU_LOCAL_AT_LEAST = 0.99


def _frames(s, second_kind):
    """match_cases.scenario()'s two frames (the same draws in the same order): frame 0 holds the object (4 x 4 cells at (2, 2)) on background;
    in frame 1 it has moved by (1, 3) cells and a second 4 x 4 region FIRES like the object, with the background's features ("distractor")
    or the object's ("twin").  -> h, w, (feat, truth, logits) of frame 0 and of frame 1"""
    H, W, S, C = s["H"], s["W"], s["stride"], s["C"]
    h, w = mc.grid_shape(H, W, S)
    rng = np.random.default_rng(s["seed"])
    proto = {k: np.maximum(rng.standard_normal(C), 0) * 2.0 for k in ("object", "background")}

    def frame(obj_cell, second_cell):
        region = np.zeros((h, w), np.int64)
        region[obj_cell[0]:obj_cell[0] + 4, obj_cell[1]:obj_cell[1] + 4] = 1
        looks = region.copy()
        if second_cell is not None and second_kind == "twin":
            looks[second_cell[0]:second_cell[0] + 4, second_cell[1]:second_cell[1] + 4] = 1
        feat = np.where(looks[..., None] == 1, proto["object"], proto["background"]) + s["noise"] * rng.standard_normal((h, w, C))
        truth = np.kron(region, np.ones((S, S), np.int64)).astype(np.uint8)
        fires = truth.copy()
        if second_cell is not None:
            fires[S * second_cell[0]:S * (second_cell[0] + 4), S * second_cell[1]:S * (second_cell[1] + 4)] = 1
        return np.maximum(feat, 0).astype(F32), truth, np.where(fires != 0, F32(2.0), F32(-2.0)).astype(F32)

    return h, w, frame((2, 2), None), frame((3, 5), s.get("twin", (7, 11)))


def _freeze(out):
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def bleed_scenario():
    """match_cases.scenario() with ONE change to the annotation: it also covers the background-looking cell BLEED["cell"], which the 3/4 rule
    then labels object.  Every background-looking distractor cell of frame 1 finds that cell at a cosine like its best background cosine, so
    with K = 1 the map is about zero there and the distractor stays; the mean over the K = 4 best foreground rows pulls three object rows in.
    -> dict with the operands, sim / map / fused (float64, tta_cases.fuse_reference) for K = 1 and K = 4, the IoUs and the margin at K = 4"""
    s = BLEED
    H, W, S, C = s["H"], s["W"], s["stride"], s["C"]
    h, w, (f0, truth0, _), (f1, truth1, logits1) = _frames(s, "distractor")
    mask0 = truth0.copy()
    mask0[S * s["cell"][0]:S * (s["cell"][0] + 1), S * s["cell"][1]:S * (s["cell"][1] + 1)] = 1
    R, rinv_r = mc.quantize(f0.reshape(h * w, C))
    label = mc.cell_labels(mask0[None], S).reshape(1, h * w)
    Q, rinv_q = mc.quantize(f1.reshape(h * w, C))
    out = dict(f0=f0, f1=f1, mask0=mask0, truth1=truth1, logits1=logits1, R=R, rinv_r=rinv_r, label=label, Q=Q, rinv_q=rinv_q, h=h, w=w,
               iou_plain=mc.iou(logits1 > 0, truth1))
    for k in (1, s["K"]):
        sim = topk(Q[None], rinv_q[None], R[None], rinv_r[None], label, k)
        mp = mc.match_map(sim).reshape(1, h, w)
        fused = tta_cases.fuse_reference([logits1[None], mp], [False, False], (H, W), [1.0, s["gain"]])
        out.update({"sim%d" % k: sim, "map%d" % k: mp, "fused%d" % k: fused, "iou%d" % k: mc.iou(fused[0] > 0, truth1),
                    "margin%d" % k: float(np.abs(fused).min())})
    return _freeze(out)


@functools.lru_cache(maxsize=None)
def twin_scenario():
    """Frame 0 is both the annotated first frame and frame t - 1: the object alone.  In frame t it has moved by (1, 3) cells and a TWIN with the
    object's features fires, TWIN["radius"] + 1 cells or more from every cell the object covered a frame ago.  First-frame matching confirms
    the twin (its features ARE the object's); the local view finds no object cell in the twin's window of the previous frame, which counts
    as cosine -1.  -> dict with the operands, the global sim / map, the local sim / idx / map, both fused logits and the IoUs"""
    s = TWIN
    H, W, S, C = s["H"], s["W"], s["stride"], s["C"]
    h, w, (f0, truth0, _), (f1, truth1, logits1) = _frames(s, "twin")
    obj = np.argwhere(truth0[::S, ::S] != 0)
    tw = np.array([(s["twin"][0] + i, s["twin"][1] + j) for i in range(4) for j in range(4)])
    assert np.abs(tw[:, None, :] - obj[None, :, :]).max(axis=2).min() >= s["radius"] + 1
    R, rinv_r = mc.quantize(f0.reshape(h * w, C))
    label = mc.cell_labels(truth0[None], S).reshape(1, h * w)
    Q, rinv_q = mc.quantize(f1.reshape(h * w, C))
    sim, _ = mc.nearest(Q[None], rinv_q[None], R[None], rinv_r[None], label)
    mp = mc.match_map(sim).reshape(1, h, w)
    lsim, lidx = local(Q[None], rinv_q[None], R[None], rinv_r[None], label, h, w, s["radius"])
    lmp = local_map(lsim).reshape(1, h, w)
    first = tta_cases.fuse_reference([logits1[None], mp], [False, False], (H, W), [1.0, s["gain"]])
    fused = tta_cases.fuse_reference([logits1[None], mp, lmp], [False, False, False], (H, W), [1.0, s["gain"], s["local_gain"]])
    return _freeze(dict(f0=f0, f1=f1, mask0=truth0, truth1=truth1, logits1=logits1, R=R, rinv_r=rinv_r, label=label, Q=Q, rinv_q=rinv_q, h=h, w=w,
                        sim=sim, map=mp, lsim=lsim, lidx=lidx, lmap=lmp, first=first, fused=fused, iou_plain=mc.iou(logits1 > 0, truth1),
                        iou_first=mc.iou(first[0] > 0, truth1), iou_local=mc.iou(fused[0] > 0, truth1)))
