#!/usr/bin/env python3
"""Generate tests/golden/boundary_f.npz: expected counts of the DAVIS boundary measure F for the cases the device kernel is tested on.

    python tests/golden/make_boundary_golden.py          # rewrites tests/golden/boundary_f.npz (needs scipy)

The counts come from a method that shares nothing with the kernel's: the boundary rule by whole-array shifts, the matches by
scipy.ndimage.binary_dilation with an explicit disk structuring element (zeros outside the image).  On four noise cases the dilation is
cross-checked against a brute-force nearest-distance search.  tests/test_boundary_f_cpu.py pins the file with a third restatement.
Layout of the file: tests/boundary_cases.py.
"""
import math
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from boundary_cases import ELLIPSE, GOLDEN, NONE, RECT, raster  # noqa: E402


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


def disk(r):
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return (x * x + y * y) <= r * r


def radius(h, w, th=0.008):
    return int(th) if th >= 1 else int(math.ceil(th * math.hypot(h, w)))


def counts(p, g, r):
    fb, gb = bmap(p), bmap(g)
    fd = ndimage.binary_dilation(fb, structure=disk(r))
    gd = ndimage.binary_dilation(gb, structure=disk(r))
    return [int((p & g).sum()), int((p | g).sum()), int(fb.sum()), int(gb.sum()), int((fb & gd).sum()), int((gb & fd).sum())]


def counts_brute(p, g, r):
    fb, gb = bmap(p), bmap(g)
    fy, fx = np.nonzero(fb)
    gy, gx = np.nonzero(gb)

    def m(ay, ax, by, bx):
        if len(ay) == 0 or len(by) == 0:
            return 0
        d = (ay[:, None] - by[None, :]) ** 2 + (ax[:, None] - bx[None, :]) ** 2
        return int((d.min(1) <= r * r).sum())
    return [int(fb.sum()), int(gb.sum()), m(fy, fx, gy, gx), m(gy, gx, fy, fx)]


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


def shapes_array(frames):
    """frames: per frame a list of (kind, a, b, c, d, roll) -> [N, S, 6], padded with NONE rows"""
    s = max(1, max(len(f) for f in frames))
    out = np.zeros((len(frames), s, 6), dtype=np.float64)
    for i, f in enumerate(frames):
        for j, row in enumerate(f):
            out[i, j] = row
    return out


def noise(rng, n, h, w, level):
    return np.stack([ndimage.gaussian_filter(rng.standard_normal((h, w)), 2) > level for _ in range(n)])


def main():
    out, names = {}, []

    def add(name, h, w, r, p=None, g=None, p_shapes=None, g_shapes=None, thr=0.5, soft=0, brute=False):
        if p is None:
            ps, gs = shapes_array(p_shapes), shapes_array(g_shapes)
            p = np.stack([raster(s, h, w) for s in ps])
            g = np.stack([raster(s, h, w) for s in gs])
            out[name + "|p_shapes"], out[name + "|g_shapes"] = ps, gs
        else:
            out[name + "|p"], out[name + "|g"] = np.packbits(p), np.packbits(g)
        n = p.shape[0]
        c = np.array([counts(p[i], g[i], r) for i in range(n)], dtype=np.int64)
        if brute:
            for i in range(n):
                assert list(c[i, 2:]) == counts_brute(p[i], g[i], r), (name, i)
        names.append(name)
        out[name + "|meta"] = np.array([n, h, w, r], dtype=np.int64)
        out[name + "|thr"] = np.float64(thr)
        out[name + "|soft"] = np.int64(soft)
        out[name + "|counts"] = c
        out[name + "|f"] = np.array([f_of(row) for row in c], dtype=np.float64)
        for i in range(n):
            print("%-18s %4dx%-4d r %2d frame %d  counts %s  F %.4f" % (name, h, w, r, i, c[i].tolist(), out[name + "|f"][i]))

    # 854x480, r = 8: an ellipse against itself rolled right by 0 / 8 / 9 / 12 / 20 px
    h, w = 480, 854
    r = radius(h, w)
    assert r == 8 and radius(1080, 1920) == 18 and radius(37, 53) == 1
    ell = (ELLIPSE, 240, 427, 120, 213)
    add("ellipse_roll", h, w, r, p_shapes=[[ell + (dx,)] for dx in (0, 8, 9, 12, 20)], g_shapes=[[ell + (0,)]] * 5)
    # a vertical edge at column 400 against one at 408 (distance r: matched) and at 409 (r + 1: not)
    add("edge_le", h, w, r, p_shapes=[[(RECT, 0, h, 0, 400 + dx, 0)] for dx in (r, r + 1)], g_shapes=[[(RECT, 0, h, 0, 400, 0)]] * 2)
    # 1920x1080, r = 18: rows AND columns tiled, shapes that touch the image border, a small blob with no counterpart
    h, w = 1080, 1920
    add("hd_shapes", h, w, radius(h, w),
        p_shapes=[[(ELLIPSE, 540, 960, 300, 500, 0), (RECT, 100, 300, 1500, 1900, 0), (RECT, 900, 1080, 0, 200, 0)],
                  [(ELLIPSE, 300, 1000, 250, 90, 0), (ELLIPSE, 800, 400, 120, 380, 0), (RECT, 0, 40, 1000, 1920, 0), (ELLIPSE, 900, 1700, 6, 9, 0)]],
        g_shapes=[[(ELLIPSE, 548, 975, 290, 510, 0), (RECT, 110, 290, 1490, 1915, 0), (RECT, 890, 1080, 0, 210, 0)],
                  [(ELLIPSE, 310, 1010, 240, 100, 0), (ELLIPSE, 790, 420, 130, 360, 25), (RECT, 0, 60, 1015, 1920, 0)]])
    # smoothed noise: widths off every word size, many small components, a halo taller than a quarter of the image
    rng = np.random.default_rng(5)
    for (h, w, rr) in [(37, 53, radius(37, 53)), (37, 53, 3), (48, 64, 5), (30, 85, 8)]:
        add("noise_%dx%d_r%d" % (h, w, rr), h, w, rr, p=noise(rng, 2, h, w, 0.0), g=noise(rng, 2, h, w, 0.1), brute=True)
    # large radii: ranges of up to three words, the built maximum
    for (h, w, rr) in [(90, 200, 40), (70, 150, 64)]:
        add("noise_%dx%d_r%d" % (h, w, rr), h, w, rr, p=noise(rng, 2, h, w, 0.3), g=noise(rng, 2, h, w, 0.4))
    # empty boundaries: all-ones against all-zeros and against itself
    for (h, w) in [(1, 1), (2, 300), (5, 7)]:
        full = (RECT, 0, h, 0, w, 0)
        add("full_%dx%d" % (h, w), h, w, radius(h, w), p_shapes=[[full], [full]], g_shapes=[[], [full]])
    # another threshold; a soft ground truth
    add("thr03_48x64_r5", 48, 64, 5, p=noise(rng, 2, 48, 64, 0.0), g=noise(rng, 2, 48, 64, 0.05), thr=0.3)
    add("softgt_37x53_r3", 37, 53, 3, p=noise(rng, 2, 37, 53, 0.0), g=noise(rng, 2, 37, 53, -0.05), soft=1)

    out["names"] = np.array(names)
    np.savez_compressed(GOLDEN, **out)
    print("wrote %s (%d bytes, %d cases)" % (GOLDEN, os.path.getsize(GOLDEN), len(names)))


if __name__ == "__main__":
    main()
