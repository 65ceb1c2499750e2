"""The softmax readout of appearance matching (csrc/match_soft.hip; the rule: include/osvos_hip.h) restated in numpy on top of
tests/match_cases.py and tests/match_ext_cases.py, with the case lists, the probes that make one bank row matter and the wide-bleed scenario,
shared by tests/test_match_soft_cpu.py and tests/test_gpu_match_soft.py.

The cosine and the exponent are restated bit for bit (single float32 operations on exact dot products); the weights 2^e and their sums are
formed in float64, the finish 1 + ln(S) / beta in float64 and rounded once.  The device may use the hardware exponential and sums in
float32, so lse is compared within ``bar``; ``best`` is match_cases.nearest's sim and is compared bit for bit."""
import functools

import numpy as np

import match_cases as mc
import match_ext_cases as me
import tta_cases

F32 = np.float32
MIN_BETA, MAX_BETA = 0.0625, 40.0
LOG2E = 1.4426950408889634                                      # log2(e), the double the host multiplies beta by
BM = BN = 128                                                   # query rows per workgroup, reference rows per tile
MAX_SLICES = 16
CHUNK = 1024                                                    # query rows per block of the restatement (memory, not arithmetic)

# ---------------------------------------------------------------------------------------------------------------- the restatement


def exponent_scale(beta):
    """k = (float) ((double) (float) beta * log2(e))"""
    return F32(np.float64(F32(beta)) * LOG2E)


def slicing(n, pq, pr):
    """-> (tiles per slice, slices): how the kernels cut the reference rows, a function of the sizes alone"""
    tiles = -(-pr // BN)
    blocks = n * -(-pq // BM)
    want = max(1, min(-(-512 // blocks), MAX_SLICES, tiles))
    tps = -(-tiles // want)
    return tps, -(-tiles // tps)


def soft(Q, rinv_q, R, rinv_r, label_r, beta):
    """the operands of match_cases.nearest and a temperature -> (lse float32 [N, 2, Pq], best float32 [N, 2, Pq]): per query row and class
    1 + ln(sum over the class's rows of 2^((cos - 1) k)) / beta, and the largest cosine; -2 for an empty class"""
    assert MIN_BETA <= beta <= MAX_BETA
    n, pq, _ = Q.shape
    nr = R.shape[0]
    assert nr in (1, n)
    k, beta64 = exponent_scale(beta), np.float64(F32(beta))
    lse = np.full((n, 2, pq), -2.0, F32)
    best = np.full((n, 2, pq), -2.0, F32)
    for b in range(n):
        rb = b if nr == n else 0
        cols = [np.flatnonzero(label_r[rb] == cls) for cls in (1, 0)]
        for a0 in range(0, pq, CHUNK):
            rq = np.asarray(rinv_q[b, a0:a0 + CHUNK], F32)
            t = mc.scores(Q[b, a0:a0 + CHUNK], R[rb], rinv_r[rb])
            cos = (t * rq[:, None]).astype(F32)
            e = ((cos - F32(1.0)).astype(F32) * k).astype(F32)
            w = np.exp2(e.astype(np.float64))
            for row in (0, 1):
                if cols[row].size == 0:
                    continue
                s = w[:, cols[row]].sum(axis=1)
                lse[b, row, a0:a0 + CHUNK] = (1.0 + np.log(s) / beta64).astype(F32)
                best[b, row, a0:a0 + CHUNK] = (t[:, cols[row]].max(axis=1) * rq).astype(F32)
    return lse, best


def soft_naive(Q, rinv_q, R, rinv_r, label_r, beta):
    """the same with Python loops and integer dots (small cases only)"""
    n, pq, _ = Q.shape
    nr = R.shape[0]
    k, beta64 = exponent_scale(beta), np.float64(F32(beta))
    lse = np.full((n, 2, pq), -2.0, F32)
    best = np.full((n, 2, pq), -2.0, F32)
    for b in range(n):
        rb = b if nr == n else 0
        for a in range(pq):
            for row, cls in ((0, 1), (1, 0)):
                s, top = 0.0, None
                for r in range(R.shape[1]):
                    if label_r[rb, r] != cls:
                        continue
                    t = F32(F32(int(np.dot(Q[b, a].astype(np.int64), R[rb, r].astype(np.int64)))) * F32(rinv_r[rb, r]))
                    cos = F32(t * F32(rinv_q[b, a]))
                    e = F32(F32(cos - F32(1.0)) * k)
                    s += 2.0 ** float(e)
                    top = t if top is None or t > top else top
                if top is not None:
                    lse[b, row, a] = F32(1.0 + np.log(s) / beta64)
                    best[b, row, a] = F32(top * F32(rinv_q[b, a]))
    return lse, best


def soft_map(lse):
    """lse [N, 2, Pq] -> lse_fg - lse_bg, float32 [N, Pq] (one float32 subtraction)"""
    return (lse[:, 0] - lse[:, 1]).astype(F32)


def class_rows(label_r):
    """label_r [NR, Pr] -> int64 [NR, 2]: the rows of the foreground and of the background"""
    return np.stack([(label_r == 1).sum(axis=1), (label_r == 0).sum(axis=1)], axis=1).astype(np.int64)


def bar(n_c, beta, lse):
    """the largest |device lse - restated lse| the rule allows: the hardware exp2 taken as good to 2 ulp (2^-22 relative) and doubled; a
    float32 sum of n positive terms off by at most (n - 1) 2^-24 relative; the error of ln S is the relative error of S, divided by beta;
    the final rounding, doubled.  Elementwise over arrays."""
    return (2.0 ** -21 + np.asarray(n_c, np.float64) * 2.0 ** -24) / float(beta) + 2.0 ** -23 * np.maximum(1.0, np.abs(np.asarray(lse, np.float64)))


def bar_of(p, beta):
    """bar for every element of a problem's lse [N, 2, Pq] (the class sizes come from its labels)"""
    n = p["lse"].shape[0]
    rows = class_rows(p["label"])
    rows = rows if rows.shape[0] == n else np.repeat(rows, n, axis=0)
    return bar(rows[:, :, None], beta, p["lse"])


# ---------------------------------------------------------------------------------------------------------------- the cases

# (Pq, Pr, C): one row; one ragged tile; across the 128-row query and reference tiles; 8 slices of one tile; 9 slices of two tiles with a
# ragged last tile of one row and rows at +-127 everywhere
SOFT_CASES = [(1, 1, 64), (37, 33, 64), (130, 257, 128), (129, 1000, 512), (300, 2049, 1024)]
SOFT_BETAS = (1.0, 10.0, 40.0)
SOFT_DAVIS_CASE = (6420, 6420, 512)
SOFT_DAVIS_BETA = 10.0
UNIFORM_PR = (127, 128, 129, 257, 2049)
PROBE_PR = 2049                                                 # 17 tiles: 9 slices of two tiles for a handful of queries


def _freeze(out):
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def soft_problem(pq, pr, c, beta, n=2, nr=1, kind="mixed"):
    """match_cases.nearest_problem's operands (duplicated rows, queries that are reference rows, dead pixels with rinv = 0, +-127 rows) with
    the restatement's (lse, best), computed once and read-only"""
    p = dict(mc.nearest_problem(pq, pr, c, n=n, nr=nr, kind=kind))
    p["lse"], p["best"] = soft(p["Q"], p["rinv_q"], p["R"], p["rinv_r"], p["label"], beta)
    return _freeze(p)


def _rows(rng, p, c=64):
    """p quantised rows of signed noise, none dead"""
    q, rinv = mc.quantize(rng.standard_normal((p, c)).astype(F32))
    assert (rinv > 0).all()
    return q, rinv


def _problem(Q, rinv_q, R, rinv_r, label, beta):
    p = dict(Q=Q[None], rinv_q=rinv_q[None], R=R[None], rinv_r=rinv_r[None], label=label[None])
    p["lse"], p["best"] = soft(p["Q"], p["rinv_q"], p["R"], p["rinv_r"], p["label"], beta)
    return _freeze(p)


@functools.lru_cache(maxsize=None)
def uniform_probe(pr, beta=1.0, pq=5):
    """every bank row is the SAME vector and the labels alternate (1, 0, 1, ..): all weights of a query are equal, so lse = cos + ln(n_c) / beta
    and a dropped or doubled row moves it by ln(1 +- 1 / n_c) / beta.  Query 0 is the bank's vector itself (cos = 1)."""
    rng = np.random.default_rng([1, pr])
    row, rinv = _rows(rng, 1)
    Q, rinv_q = _rows(rng, pq)
    Q[0], rinv_q[0] = row[0], rinv[0]
    label = (1 - np.arange(pr) % 2).astype(np.uint8)
    return _problem(Q, rinv_q, np.repeat(row, pr, axis=0), np.repeat(rinv, pr), label, beta)


def hot_rows(pr=PROBE_PR, pq=3):
    """where one hot row is planted: the first and the last row of the first tile, the first of the second, the last of the bank, and the
    first row of the second slice"""
    tps, slices = slicing(1, pq, pr)
    assert slices > 1
    return (0, BN - 1, BN, pr - 1, tps * BN)


@functools.lru_cache(maxsize=None)
def hot_probe(b, void=False, pr=PROBE_PR, beta=40.0, pq=3):
    """every bank row is the NEGATIVE of query 0 (cosine -1: weight exp(-2 beta)) but row ``b``, which IS query 0 (cosine 1: weight 1); the
    labels alternate.  At beta 40 the hot row alone decides its class: lse is about 1 with it and about -1 + ln(n_c) / beta without.
    ``void``: the hot row carries label 255 and must contribute to neither class."""
    rng = np.random.default_rng([2, pr])
    Q, rinv_q = _rows(rng, pq)
    R, rinv_r = np.repeat(-Q[:1], pr, axis=0), np.repeat(rinv_q[:1], pr)
    R[b] = Q[0]
    label = (1 - np.arange(pr) % 2).astype(np.uint8)
    if void:
        label[b] = mc.VOID
    return _problem(Q, rinv_q, R, rinv_r, label, beta)


# ---------------------------------------------------------------------------------------------------------------- the scenario

WIDE = dict(me.BLEED, gain=8.0, topk_gain=me.BLEED["gain"], beta=10.0, cells=((6, 3), (6, 4), (7, 3), (7, 4)), K=4)
WIDE_IOU_PLAIN = 0.5
# top-K is pinned at BOTH gains.  At the bleed scenario's own gain (6) K = 1 and K = 4 leave the distractor whole: IoU 0.5 (K = 8 gives 0.71).
# At the soft readout's gain (8) they leave it too, and the stronger map also lifts a rim of pixels around the object over zero: 1121 false
# pixels in place of 1024.
WIDE_IOU_K1 = 0.5
WIDE_IOU_K4 = 0.5
WIDE_IOU_K1_AT_SOFT_GAIN = WIDE_IOU_K4_AT_SOFT_GAIN = 1024.0 / 2145.0
WIDE_IOU_SOFT = 1.0                                             # (at gain 8; the soft readout at gain 6 gives 1.0 as well, margin 0.18)
WIDE_MARGIN_SOFT = 0.905                                        # smallest |fused logit| under the soft readout, to three digits


@functools.lru_cache(maxsize=None)
def wide_bleed_scenario():
    """match_ext_cases.bleed_scenario() with a WIDER mistake in the annotation: it covers a 2 x 2 block of background-looking cells, which the
    3/4 rule labels object.  Four mislabelled rows are as many as topk averages at K = 4, so the mean of the four best foreground rows of a
    distractor cell is still their cosine and the distractor stays; under the softmax readout the four rows are outvoted by the mass of the
    background rows that look the same.  -> dict with the operands, sim / map / fused for K = 1 and K = 4, lse / best / map / fused for the
    soft readout (float64 fusion, tta_cases.fuse_reference), the IoUs and the soft margin"""
    s = WIDE
    H, W, S, C = s["H"], s["W"], s["stride"], s["C"]
    h, w, (f0, truth0, _), (f1, truth1, logits1) = me._frames(s, "distractor")
    mask0 = truth0.copy()
    for i, j in s["cells"]:
        mask0[S * i:S * (i + 1), S * j:S * (j + 1)] = 1
    R, rinv_r = mc.quantize(f0.reshape(h * w, C))
    label = mc.cell_labels(mask0[None], S).reshape(1, h * w)
    Q, rinv_q = mc.quantize(f1.reshape(h * w, C))
    out = dict(f0=f0, f1=f1, mask0=mask0, truth1=truth1, logits1=logits1, R=R, rinv_r=rinv_r, label=label, Q=Q, rinv_q=rinv_q, h=h, w=w,
               iou_plain=mc.iou(logits1 > 0, truth1))

    def fuse(mp, gain=s["gain"]):
        return tta_cases.fuse_reference([logits1[None], mp], [False, False], (H, W), [1.0, gain])

    for k in (1, s["K"]):
        sim = me.topk(Q[None], rinv_q[None], R[None], rinv_r[None], label, k)
        mp = mc.match_map(sim).reshape(1, h, w)
        out.update({"sim%d" % k: sim, "iou_k%d" % k: mc.iou(fuse(mp, s["topk_gain"])[0] > 0, truth1),
                    "iou_k%d_at_soft_gain" % k: mc.iou(fuse(mp)[0] > 0, truth1)})
    lse, best = soft(Q[None], rinv_q[None], R[None], rinv_r[None], label, s["beta"])
    mp = soft_map(lse).reshape(1, h, w)
    fused = fuse(mp)
    out.update(lse=lse, best=best, map_soft=mp, fused_soft=fused, iou_soft=mc.iou(fused[0] > 0, truth1), margin_soft=float(np.abs(fused).min()))
    return _freeze(out)
