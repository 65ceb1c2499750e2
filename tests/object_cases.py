"""Shared by the multi-object tests and tests/golden/make_objects_golden.py: reads tests/golden/objects.npz and turns a case into the label
maps and the logit stack a test feeds to the device.  Nothing here merges logits, computes a boundary or a match.

Fixture layout (one entry per case name in ``names``):
    <name>|meta     int64 [5]         N, K, H, W, matching radius r in pixels
    <name>|thr      float64           probability threshold of the merge (0.5 unless the case says otherwise)
    <name>|special  int64 [M, 6]      rows (n, y, x, kind, a, b): pixels whose logits ``logits`` sets by hand, see the kinds below
    <name>|counts   int64 [N, K, 6]   per frame and object id k = 1..K: |P & G|, |P | G|, |B(P)|, |B(G)|, matched of B(P), matched of B(G)
                                      with P = (pred == k), G = (gt == k)
    label maps, either  <name>|pred, <name>|gt                  uint8 [N, H, W]
    or                  <name>|pred_shapes, <name>|gt_shapes    float64 [N, S, 7] rows (kind, a, b, c, d, roll, id), see ``raster``
``pred`` is what the merge of ``logits(case)`` must give; ``gt`` may hold ids above K, which belong to no object.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "objects.npz")
NONE, ELLIPSE, RECT = 0, 1, 2
# kinds of special pixels
TIE = 1        # objects a < b share the maximum exactly: the label is a
THR_EQ = 2     # the maximum (object a's logit) EQUALS the logit threshold: background
NAN = 3        # object a's logit is NaN; the other objects decide the pixel as they would without it
ALL_NAN = 4    # every logit is NaN: background


def raster(shapes, h, w):
    """Label map of one frame: the shapes painted in order, a later one over an earlier one.  ELLIPSE: centre (a, b), semi-axes (c, d) in
    (row, column) order, pixels with ((y - a) / c)^2 + ((x - b) / d)^2 <= 1; RECT: rows [a, b), columns [c, d); each rolled right by
    `roll` columns (np.roll) and filled with `id`."""
    yy, xx = np.mgrid[:h, :w]
    m = np.zeros((h, w), dtype=np.uint8)
    for kind, a, b, c, d, roll, ident in np.asarray(shapes, dtype=np.float64).reshape(-1, 7):
        if int(kind) == ELLIPSE:
            s = (((yy - a) / c) ** 2 + ((xx - b) / d) ** 2) <= 1
        elif int(kind) == RECT:
            s = (yy >= a) & (yy < b) & (xx >= c) & (xx < d)
        else:
            continue
        m[np.roll(s, int(roll), axis=1)] = int(ident)
    return m


def load(path=GOLDEN):
    z = np.load(path)
    cases = []
    for name in [str(s) for s in z["names"]]:
        n, k, h, w, r = [int(v) for v in z[name + "|meta"]]
        c = {"name": name, "N": n, "K": k, "H": h, "W": w, "r": r, "thr": float(z[name + "|thr"]),
             "special": z[name + "|special"].astype(np.int64).reshape(-1, 6), "counts": z[name + "|counts"].astype(np.int64)}
        for key in ("pred", "gt"):
            if name + "|" + key in z.files:
                c[key] = z[name + "|" + key].astype(np.uint8)
            else:
                c[key] = np.stack([raster(s, h, w) for s in z[name + "|" + key + "_shapes"]])
        cases.append(c)
    return cases


def logit_threshold(thr):
    return np.float32(np.log(thr / (1.0 - thr)))


def logits(case, seed=0):
    """float32 [K, N, H, W] whose merge is the case's ``pred``: where pred == k object k's logit sits above the logit threshold t by 1e-3 .. ~8
    and every other object's sits below the WINNER by at least 1e-3 (on either side of t); where pred == 0 every logit sits below t by at
    least 1e-3.  Then the special pixels are set by hand (see the kinds)."""
    rng = np.random.default_rng(2000 + seed)
    pred, k, t = case["pred"], case["K"], logit_threshold(case["thr"])
    shape = pred.shape
    win = (t + np.float32(1e-3) + (8.0 * rng.random(shape) ** 3).astype(np.float32)).astype(np.float32)
    x = np.empty((k,) + shape, dtype=np.float32)
    for j in range(k):
        below = (np.float32(1e-3) + (6.0 * rng.random(shape) ** 2).astype(np.float32)).astype(np.float32)
        x[j] = np.where(pred == j + 1, win, np.where(pred == 0, t - below, win - below))
    for n, y, xx, kind, a, b in case["special"]:
        if kind == TIE:
            x[b - 1, n, y, xx] = x[a - 1, n, y, xx]
        elif kind == THR_EQ:
            x[a - 1, n, y, xx] = t
        elif kind == NAN:
            x[a - 1, n, y, xx] = np.nan
        elif kind == ALL_NAN:
            x[:, n, y, xx] = np.nan
        else:
            raise ValueError("special pixel kind %d" % kind)
    return x
