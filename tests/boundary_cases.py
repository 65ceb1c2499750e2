"""Shared by the boundary-measure tests and tests/golden/make_boundary_golden.py: reads tests/golden/boundary_f.npz and turns a case
into the masks and the float tensors a test feeds to the device.  Nothing here computes a boundary or a match.

Fixture layout (one entry per case name in ``names``):
    <name>|meta     int64 [4]      N, H, W, matching radius r in pixels
    <name>|thr      float64        probability threshold of the prediction (0.5 unless the case says otherwise)
    <name>|soft     int64          1: the ground truth is fed as soft values around 0.5 instead of 0 / 1
    <name>|counts   int64 [N, 6]   |P & G|, |P | G|, |B(P)|, |B(G)|, matched of B(P), matched of B(G)
    <name>|f        float64 [N]    F of the generator's own run
    masks, either   <name>|p, <name>|g                 uint8, np.packbits of the bool array [N, H, W]
    or              <name>|p_shapes, <name>|g_shapes   float64 [N, S, 6] rows (kind, a, b, c, d, roll): procedural masks, see ``raster``
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boundary_f.npz")
NONE, ELLIPSE, RECT = 0, 1, 2


def raster(shapes, h, w):
    """Union of the shapes of one frame.  ELLIPSE: centre (a, b), semi-axes (c, d) in (row, column) order, pixels with
    ((y - a) / c)^2 + ((x - b) / d)^2 <= 1; RECT: rows [a, b), columns [c, d).  Each shape is then rolled right by `roll`
    columns (np.roll: what leaves on the right comes back on the left)."""
    yy, xx = np.mgrid[:h, :w]
    m = np.zeros((h, w), dtype=bool)
    for kind, a, b, c, d, roll in np.asarray(shapes, dtype=np.float64).reshape(-1, 6):
        if int(kind) == ELLIPSE:
            s = (((yy - a) / c) ** 2 + ((xx - b) / d) ** 2) <= 1
        elif int(kind) == RECT:
            s = (yy >= a) & (yy < b) & (xx >= c) & (xx < d)
        else:
            continue
        m |= np.roll(s, int(roll), axis=1)
    return m


def load(path=GOLDEN):
    z = np.load(path)
    cases = []
    for name in [str(s) for s in z["names"]]:
        n, h, w, r = [int(v) for v in z[name + "|meta"]]
        c = {"name": name, "N": n, "H": h, "W": w, "r": r, "thr": float(z[name + "|thr"]), "soft": int(z[name + "|soft"]),
             "counts": z[name + "|counts"].astype(np.int64), "f": z[name + "|f"].astype(np.float64)}
        for key in ("p", "g"):
            if name + "|" + key in z.files:
                c[key] = np.unpackbits(z[name + "|" + key], count=n * h * w).reshape(n, h, w).astype(bool)
            else:
                c[key] = np.stack([raster(s, h, w) for s in z[name + "|" + key + "_shapes"]])
        cases.append(c)
    return cases


def tensors(case, seed=0):
    """float32 arrays (logits [N,1,H,W], gt [N,1,H,W]) whose thresholded masks are the case's: logits sit on both sides of the logit
    threshold at distances from 1e-3 to ~8 that vary per pixel; a soft ground truth takes values in (0.5, 1] where the mask is set and in
    [0, 0.5] -- the value 0.5 itself included: `gt > 0.5` is strict -- where it is not."""
    rng = np.random.default_rng(1000 + seed)
    shape = case["p"].shape
    t = np.float32(np.log(case["thr"] / (1.0 - case["thr"])))
    mag = (1e-3 + 8.0 * rng.random(shape) ** 3).astype(np.float32)
    logits = np.where(case["p"], t + mag, t - mag).astype(np.float32)
    assert np.array_equal(logits > t, case["p"])
    if case["soft"]:
        u = rng.random(shape).astype(np.float32)
        lo = np.where(rng.random(shape) < 0.25, np.float32(0.5), np.float32(0.5) * u)
        hi = np.float32(0.5) + np.maximum(np.float32(0.5) * u, np.float32(1e-6))
        gt = np.where(case["g"], hi, lo).astype(np.float32)
    else:
        gt = case["g"].astype(np.float32)
    assert np.array_equal(gt > np.float32(0.5), case["g"])
    return logits[:, None], gt[:, None]
