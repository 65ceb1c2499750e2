#!/usr/bin/env python3
"""Generate tests/golden/objects.npz: label maps, special pixels and expected per-object counts for the multi-object kernels
(osvos_merge_objects, osvos_labels_jf_counts; csrc/objects.hip).

    python tests/golden/make_objects_golden.py          # rewrites tests/golden/objects.npz (numpy only)

Everything is restated here in plain numpy, sharing nothing with the kernels: the merge as fmax / first-argmax over the object axis, the
boundary by the neighbour rule on whole-array shifts, the matches by a brute-force nearest-distance search between the two boundary pixel
lists.  The label maps are designed first (shapes or smoothed-noise arg-max maps plus hand-placed special pixels), tests/object_cases.py
builds the logits from them, and the merge of those logits -- which must give the designed map back -- is what the file stores.
Layout of the file: tests/object_cases.py.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import object_cases as oc  # noqa: E402
from object_cases import ALL_NAN, ELLIPSE, GOLDEN, NAN, RECT, THR_EQ, TIE  # noqa: E402


def merge(x, t):
    """[K, N, H, W] float32 -> uint8 [N, H, W] by the definition in include/osvos_hip.h"""
    m = np.fmax.reduce(x, axis=0)                              # fmax: NaN only where every logit is NaN
    with np.errstate(invalid="ignore"):
        fg = m > t                                             # NaN compares false
        first = np.argmax(x == m[None], axis=0)                # lowest k with logits[k] == m (NaN == m is false)
    return np.where(fg, first + 1, 0).astype(np.uint8)


def bmap(seg):
    seg = seg.astype(bool)
    e, s, se = np.zeros_like(seg), np.zeros_like(seg), np.zeros_like(seg)
    e[:, :-1] = seg[:, 1:]
    s[:-1, :] = seg[1:, :]
    se[:-1, :-1] = seg[1:, 1:]
    b = (seg ^ e) | (seg ^ s) | (seg ^ se)
    b[-1, :] = seg[-1, :] ^ e[-1, :]
    b[:, -1] = seg[:, -1] ^ s[:, -1]
    b[-1, -1] = False
    return b


def matched(a, b, r):
    """pixels of boundary map a that have a pixel of b within distance r (brute force, in row chunks)"""
    ay, ax = np.nonzero(a)
    by, bx = np.nonzero(b)
    if len(ay) == 0 or len(by) == 0:
        return 0
    n = 0
    for s in range(0, len(ay), 512):
        d = (ay[s:s + 512, None] - by[None, :]) ** 2 + (ax[s:s + 512, None] - bx[None, :]) ** 2
        n += int((d.min(1) <= r * r).sum())
    return n


def counts(p, g, r):
    fb, gb = bmap(p), bmap(g)
    return [int((p & g).sum()), int((p | g).sum()), int(fb.sum()), int(gb.sum()), matched(fb, gb, r), matched(gb, fb, r)]


def f_of(c):
    nf, ng, mf, mg = c[2:]
    if nf == 0 and ng > 0:
        pr, rc = 1.0, 0.0
    elif nf > 0 and ng == 0:
        pr, rc = 0.0, 1.0
    elif nf == 0 and ng == 0:
        pr, rc = 1.0, 1.0
    else:
        pr, rc = mf / nf, mg / ng
    return 0.0 if pr + rc == 0 else 2 * pr * rc / (pr + rc)


def radius(h, w, th=0.008):
    return int(th) if th >= 1 else int(math.ceil(th * math.hypot(h, w)))


def smooth(a, passes):
    for _ in range(passes):
        a = (a + np.roll(a, 1, 0) + np.roll(a, -1, 0) + np.roll(a, 1, 1) + np.roll(a, -1, 1)) / 5.0
    return a


def noise_labels(rng, n, h, w, ids, level, passes=20):
    """arg-max map of smoothed noise fields, one per id in `ids`; background where the winner stays under `level` standard deviations"""
    out = np.zeros((n, h, w), dtype=np.uint8)
    for i in range(n):
        f = np.stack([smooth(rng.standard_normal((h, w)), passes) for _ in ids])
        f /= f.std()
        out[i] = np.where(f.max(0) > level, np.asarray(ids, dtype=np.uint8)[f.argmax(0)], 0)
    return out


def shapes_array(frames):
    s = max(1, max(len(f) for f in frames))
    out = np.zeros((len(frames), s, 7), dtype=np.float64)
    for i, f in enumerate(frames):
        for j, row in enumerate(f):
            out[i, j] = row
    return out


def pick_specials(rng, pred, k, ties, thr_eq, nans, all_nans):
    """special pixels that leave the designed map `pred` as the answer: ties at pixels of an object a < K (with some b > a), the other
    kinds as object_cases describes them"""
    rows, used = [], set()

    def take(mask, count):
        idx = np.argwhere(mask)
        got = []
        if count == 0:
            return got
        for j in rng.permutation(len(idx)):
            key = tuple(int(v) for v in idx[j])
            if key not in used:
                used.add(key)
                got.append(key)
            if len(got) == count:
                break
        return got
    if k >= 2:
        for (n, y, x) in take((pred > 0) & (pred < k), ties):
            a = int(pred[n, y, x])
            rows.append((n, y, x, TIE, a, int(rng.integers(a + 1, k + 1))))
    for (n, y, x) in take(pred == 0, thr_eq):
        rows.append((n, y, x, THR_EQ, int(rng.integers(1, k + 1)), 0))
    if k >= 2:
        for (n, y, x) in take(np.ones_like(pred, dtype=bool), nans):
            a = int(rng.integers(1, k + 1))
            while a == int(pred[n, y, x]):
                a = int(rng.integers(1, k + 1))
            rows.append((n, y, x, NAN, a, 0))
    for (n, y, x) in take(pred == 0, all_nans):
        rows.append((n, y, x, ALL_NAN, 0, 0))
    return np.array(rows, dtype=np.int64).reshape(-1, 6)


def main():
    out, names, with_ties = {}, [], 0
    rng = np.random.default_rng(17)

    def add(name, k, h, w, r, pred=None, gt=None, pred_shapes=None, gt_shapes=None, thr=0.5, ties=0, thr_eq=0, nans=0, all_nans=0):
        nonlocal with_ties
        if pred is None:
            ps, gs = shapes_array(pred_shapes), shapes_array(gt_shapes)
            pred = np.stack([oc.raster(s, h, w) for s in ps])
            gt = np.stack([oc.raster(s, h, w) for s in gs])
            out[name + "|pred_shapes"], out[name + "|gt_shapes"] = ps, gs
        else:
            out[name + "|pred"], out[name + "|gt"] = pred, gt
        n = pred.shape[0]
        assert pred.shape == gt.shape == (n, h, w) and pred.max() <= k
        special = pick_specials(rng, pred, k, ties, thr_eq, nans, all_nans)
        case = {"name": name, "N": n, "K": k, "H": h, "W": w, "r": r, "thr": thr, "special": special, "pred": pred, "gt": gt}
        x = oc.logits(case)
        assert x.shape == (k, n, h, w) and x.dtype == np.float32
        assert np.array_equal(merge(x, oc.logit_threshold(thr)), pred), name          # the designed map IS the merge of the built logits
        n_ties = int((special[:, 3] == TIE).sum())
        for row in special[special[:, 3] == TIE]:
            assert x[row[4] - 1, row[0], row[1], row[2]] == x[row[5] - 1, row[0], row[1], row[2]] and row[4] < row[5]
        assert n_ties == (ties if k >= 2 else 0)
        with_ties += n_ties > 0
        c = np.array([[counts(pred[i] == j, gt[i] == j, r) for j in range(1, k + 1)] for i in range(n)], dtype=np.int64)
        fs = np.array([[f_of(row) for row in frame] for frame in c])
        assert ((fs > 0) & (fs < 1)).any(), name                                        # the case is not a trivial one
        names.append(name)
        out[name + "|meta"] = np.array([n, k, h, w, r], dtype=np.int64)
        out[name + "|thr"] = np.float64(thr)
        out[name + "|special"] = special
        out[name + "|counts"] = c
        for i in range(n):
            for j in range(k):
                print("%-18s %4dx%-4d r %2d frame %d object %2d  counts %s  F %.4f" % (name, h, w, r, i, j + 1, c[i, j].tolist(), fs[i, j]))
        return c

    # K = 1: the single-object measure through the label path; width 53
    add("k1_37x53", 1, 37, 53, 2, pred=noise_labels(rng, 2, 37, 53, [1], 0.0), gt=noise_labels(rng, 2, 37, 53, [1], 0.1), thr_eq=3, all_nans=2)
    # K = 2: two rectangles that TOUCH along a column and an ellipse painted OVER both; the ground truth moved a little
    add("k2_touch_48x64", 2, 48, 64, 3,
        pred_shapes=[[(RECT, 8, 40, 6, 30, 0, 1), (RECT, 8, 40, 30, 58, 0, 2), (ELLIPSE, 24, 30, 9, 12, 0, 1)],
                     [(RECT, 4, 30, 2, 33, 0, 2), (ELLIPSE, 30, 40, 14, 20, 0, 1)]],
        gt_shapes=[[(RECT, 9, 42, 4, 31, 0, 1), (RECT, 9, 42, 31, 60, 0, 2), (ELLIPSE, 25, 33, 8, 11, 0, 1)],
                   [(RECT, 5, 28, 4, 30, 0, 2), (ELLIPSE, 29, 43, 13, 18, 0, 1)]],
        ties=12, thr_eq=4, nans=6)
    # K = 3, width 85, r = 8 (a halo taller than a quarter of the image): noise maps; object 3 never predicted in frame 0 ...
    p = noise_labels(rng, 2, 30, 85, [1, 2, 3], 0.4)
    g = noise_labels(rng, 2, 30, 85, [1, 2, 3], 0.5)
    p[0][p[0] == 3] = 0
    g[1][g[1] == 2] = 0                                                                 # ... and object 2 absent from the ground truth of frame 1
    add("k3_30x85_r8", 3, 30, 85, 8, pred=p, gt=g, ties=10, nans=5, all_nans=2)
    # K = 10, width 107, a threshold other than 0.5: ids 1..9 in the prediction (10 in neither map: missing from both; 9 missing from the
    # ground truth; 8 missing from the prediction of frame 1), ground-truth ids 11 and 12 above K
    p = noise_labels(rng, 2, 60, 107, list(range(1, 10)), 0.3, passes=10)
    g = noise_labels(rng, 2, 60, 107, [1, 2, 3, 4, 5, 6, 7, 8, 11, 12], 0.3, passes=10)
    p[1][p[1] == 8] = 0
    add("k10_60x107_thr03", 10, 60, 107, radius(60, 107), pred=p, gt=g, thr=0.3, ties=16, thr_eq=5, nans=8)
    # K = 16, the built maximum: every lane of the pack kernel's hand-over is used; ground-truth id 17 above K
    p = noise_labels(rng, 1, 40, 150, list(range(1, 17)), 0.2, passes=8)
    g = np.roll(p, 2, axis=2)
    g[g == 5] = 17
    add("k16_40x150", 16, 40, 150, 4, pred=p, gt=g, thr=0.7, ties=8, nans=10, all_nans=3, thr_eq=5)
    # one 854x480 frame, r = 8, K = 3: overlapping ellipses against moved ones, a shape on the image border
    h, w = 480, 854
    assert radius(h, w) == 8
    add("davis_854x480", 3, h, w, 8,
        pred_shapes=[[(ELLIPSE, 240, 300, 120, 160, 0, 1), (ELLIPSE, 260, 480, 100, 140, 0, 2), (RECT, 400, 480, 700, 854, 0, 3)]],
        gt_shapes=[[(ELLIPSE, 244, 309, 118, 150, 0, 1), (ELLIPSE, 255, 470, 104, 150, 12, 2), (RECT, 390, 480, 712, 854, 0, 3)]],
        ties=20, thr_eq=6, nans=10, all_nans=2)

    assert with_ties >= 3
    assert sorted(set(int(out[n + "|meta"][1]) for n in names)) == [1, 2, 3, 10, 16]
    out["names"] = np.array(names)
    np.savez_compressed(GOLDEN, **out)
    size = os.path.getsize(GOLDEN)
    print("wrote %s (%d bytes, %d cases)" % (GOLDEN, size, len(names)))
    assert size < 200 * 1024


if __name__ == "__main__":
    main()
