"""Writes tests/golden/components.npz: masks, their canonical connected-component labellings under 4- and 8-connectivity, areas and
stats, and the expected outputs of the selection rule on a tracking sequence.  (Layout: tests/component_cases.py.)

Shares no code with the product.  Labelling is restated as a plain breadth-first flood fill in raster order, the selection rule is
restated literally from include/osvos_hip.h, and every labelling is compared with scipy.ndimage.label (structure ones((3, 3)) for
8-connectivity, the default cross for 4) renumbered by first appearance in raster order; on any disagreement nothing is written.

    python tests/golden/make_components_golden.py
"""
import os
import sys
from collections import deque

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import component_cases as cc  # noqa: E402

NEIGHBOURS = {4: [(-1, 0), (1, 0), (0, -1), (0, 1)],
              8: [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]}


def flood_labels(mask, conn):
    """canonical labels of one frame: raster scan, a pixel not yet labelled starts a fill; its flat index is the lowest of its component"""
    h, w = mask.shape
    lab = np.zeros((h, w), dtype=np.int32)
    for y in range(h):
        for x in range(w):
            if not mask[y, x] or lab[y, x]:
                continue
            ident = y * w + x + 1
            lab[y, x] = ident
            q = deque([(y, x)])
            while q:
                cy, cx = q.popleft()
                for dy, dx in NEIGHBOURS[conn]:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < h and 0 <= nx < w and mask[ny, nx] and not lab[ny, nx]:
                        lab[ny, nx] = ident
                        q.append((ny, nx))
    return lab


def renumbered(lab):
    """labels replaced by the rank of their first appearance in raster order (1, 2, ..)"""
    flat = lab.reshape(-1)
    out = np.zeros_like(flat)
    seen = {}
    for i, v in enumerate(flat):
        if v:
            out[i] = seen.setdefault(int(v), len(seen) + 1)
    return out.reshape(lab.shape)


def check_against_scipy(mask, lab, conn):
    ref, count = ndimage.label(mask, structure=np.ones((3, 3)) if conn == 8 else None)
    if not np.array_equal(renumbered(lab), renumbered(ref)):
        raise SystemExit("flood fill and scipy.ndimage.label disagree: nothing written")
    ids = np.unique(lab[lab > 0])
    assert len(ids) == count and np.array_equal(np.sort(ids), ids)


def area_and_stats(lab):
    h, w = lab.shape
    area = np.zeros((h, w), dtype=np.int32)
    ids, counts = np.unique(lab[lab > 0], return_counts=True)
    for i, c in zip(ids, counts):
        area.reshape(-1)[i - 1] = c
    stats = np.zeros(4, dtype=np.int64)
    if len(ids):
        best = int(counts.max())
        stats[:] = [len(ids), int(counts.sum()), best, int(ids[counts == best].min())]
    return area, stats


def select(mask, lab, seed, chain, radius, min_area, keep_largest):
    """the rule of include/osvos_hip.h, component by component -> kept [N, H, W] bool"""
    n_frames = mask.shape[0]
    kept = np.zeros_like(mask)
    for n in range(n_frames):
        s = None if seed is None else (seed[0] if chain and n == 0 else kept[n - 1] if chain else seed[n])
        ids, counts = np.unique(lab[n][lab[n] > 0], return_counts=True)
        largest = int(ids[counts == counts.max()].min()) if len(ids) else 0
        sy, sx = np.nonzero(s) if s is not None else (np.zeros(0, int), np.zeros(0, int))
        for ident, count in zip(ids, counts):
            if count < min_area:
                continue
            if keep_largest and ident != largest:
                continue
            if s is not None and len(sy):
                py, px = np.nonzero(lab[n] == ident)
                d2 = (py[:, None] - sy[None, :]) ** 2 + (px[:, None] - sx[None, :]) ** 2
                if not (d2 <= radius * radius).any():
                    continue
            kept[n][lab[n] == ident] = True
    return kept


def ellipse(h, w, cy, cx, ry, rx):
    yy, xx = np.mgrid[:h, :w]
    return (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) <= 1


def spiral(h, w, pitch=4):
    """a one-pixel square spiral from (0, 0) inwards, its arms `pitch` pixels apart"""
    m = np.zeros((h, w), dtype=bool)
    k = 0
    while True:
        t, b, l, r = k * pitch, h - 1 - k * pitch, k * pitch, w - 1 - k * pitch
        if b - t < pitch or r - l < pitch:
            break
        m[t, (l - pitch if k else l):r + 1] = True      # right (from the end of the previous ring's way up)
        m[t:b + 1, r] = True                            # down
        m[b, l:r + 1] = True                            # left
        m[t + pitch:b + 1, l] = True                    # up, to where the next ring starts
        k += 1
    return m


def special_pixels(mask, rng):
    """up to three background pixels per kind and frame, next to the foreground where there is any: would they count as foreground,
    the components would change"""
    rows = []
    for n in range(mask.shape[0]):
        near = ndimage.binary_dilation(mask[n], structure=np.ones((3, 3))) & ~mask[n]
        cand = np.argwhere(near if near.any() else ~mask[n])
        if len(cand) == 0:
            continue
        pick = cand[rng.permutation(len(cand))[:6]]
        for i, (y, x) in enumerate(pick):
            rows.append((n, int(y), int(x), cc.THR_EQ if i % 2 == 0 else cc.NAN))
    return np.array(rows, dtype=np.int64).reshape(-1, 4)


def build_cases():
    cases = []

    def add(name, mask, thr=0.5):
        cases.append({"name": name, "mask": np.asarray(mask, dtype=bool), "thr": thr})

    m = np.zeros((2, 30, 85), dtype=bool)
    m[1] = True
    add("empty_full_30x85", m)

    m = np.zeros((1, 37, 53), dtype=bool)
    for y, x in [(0, 0), (36, 52), (0, 52), (18, 26)]:
        m[0, y, x] = True
    add("single_pixels_37x53", m)

    m = np.zeros((2, 16, 16), dtype=bool)
    m[0][np.arange(16), np.arange(16)] = True
    yy, xx = np.mgrid[:16, :16]
    m[1] = (yy + xx) % 2 == 0
    add("diagonal_checker_16x16", m)

    m = np.zeros((2, 37, 53), dtype=bool)
    m[0, 36, :] = True
    m[1, 0, :] = True
    add("two_frames_37x53", m)

    m = np.zeros((1, 150, 300), dtype=bool)
    m[0, 0::2, :] = True
    m[0, 1::4, 299] = True
    m[0, 3::4, 0] = True
    add("serpentine_150x300", m)

    m = np.zeros((1, 96, 200), dtype=bool)
    m[0, :, 0::2] = True
    m[0, 95, :] = True
    add("comb_96x200", m)

    m = np.zeros((1, 65, 129), dtype=bool)
    m[0] = spiral(65, 129)
    m[0, 2:63, 2:127] |= spiral(61, 125)
    add("spiral_65x129", m)

    rng = np.random.default_rng(20171)
    m = rng.random((1, 64, 128)) < 0.45
    for x0 in (2, 20):                                   # two equal blobs behind a moat: a tie for the largest area under 4-connectivity
        m[0, 1:14, x0 - 1:x0 + 12] = False
        m[0, 2:13, x0:x0 + 11] = True
    add("noise_64x128", m)
    add("noise_60x107_thr03", rng.random((1, 60, 107)) < 0.60, thr=0.3)

    m = np.zeros((1, 48, 64), dtype=bool)
    m[0] = ellipse(48, 64, 24, 32, 20, 26) & ~ellipse(48, 64, 24, 32, 16, 22)
    m[0] |= ellipse(48, 64, 24, 32, 6, 8)
    add("ring_blob_48x64", m)
    return cases


def tracking_case():
    n, h, w, radius = 8, 48, 64, 3
    mask = np.zeros((n, h, w), dtype=bool)
    obj = np.zeros((n, h, w), dtype=bool)
    for f in range(n):
        cx = 14 + 2 * f
        if f != 4:                                       # frame 4: the object is absent
            obj[f] = ellipse(h, w, 24, cx, 8, 6)
            mask[f] |= obj[f]
            mask[f, 24:26, cx + 8] = True                # a speck of two pixels, one pixel away from the object
        if f >= 2:
            mask[f, 6:13, 48:57] = True                  # the distractor, far from the object
    return {"name": "track", "mask": mask, "thr": 0.5}, obj, radius


def main():
    out = {}
    cases = build_cases()
    track, obj, radius = tracking_case()
    cases.append(track)
    rng = np.random.default_rng(7)
    ties = 0
    for c in cases:
        name, mask = c["name"], c["mask"]
        n, h, w = mask.shape
        c["special"] = special_pixels(mask, rng)
        assert not any(mask[r[0], r[1], r[2]] for r in c["special"])
        out[name + "|meta"] = np.array([n, h, w], dtype=np.int64)
        out[name + "|thr"] = np.float64(c["thr"])
        out[name + "|mask"] = cc.pack(mask)
        out[name + "|special"] = c["special"]
        x = cc.logits(c)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(x > cc.logit_threshold(c["thr"]), mask), name      # the logits threshold back to the mask
        per = {}
        for conn in (4, 8):
            lab = np.stack([flood_labels(mask[f], conn) for f in range(n)])
            for f in range(n):
                check_against_scipy(mask[f], lab[f], conn)
            a_s = [area_and_stats(lab[f]) for f in range(n)]
            per[conn] = (lab, np.stack([a for a, _ in a_s]), np.stack([s for _, s in a_s]))
            for f in range(n):
                areas = per[conn][1][f][per[conn][1][f] > 0]
                ties += len(areas) > 1 and int((areas == areas.max()).sum()) > 1 and name.startswith("noise")
        c["per"] = per
        same = all(np.array_equal(per[4][i], per[8][i]) for i in range(3))
        for conn in (4,) if same else (4, 8):
            out["%s|labels%d" % (name, conn)], out["%s|area%d" % (name, conn)], out["%s|stats%d" % (name, conn)] = per[conn]
        print("%-24s N %d  %3d x %3d  components 4: %-22s 8: %s" % (name, n, h, w, per[4][2][:, 0].tolist(), per[8][2][:, 0].tolist()))

    by = {c["name"]: c for c in cases}
    assert ties >= 1, "no tie for the largest area in a noise case"
    assert by["empty_full_30x85"]["per"][8][2].tolist() == [[0, 0, 0, 0], [1, 30 * 85, 30 * 85, 1]]
    assert by["single_pixels_37x53"]["per"][4][2].tolist() == [[4, 4, 1, 1]]
    d = by["diagonal_checker_16x16"]["per"]
    assert d[4][2][:, 0].tolist() == [16, 128] and d[8][2][:, 0].tolist() == [1, 1]
    assert by["two_frames_37x53"]["per"][8][2][:, 0].tolist() == [1, 1]
    s = by["serpentine_150x300"]["per"]
    assert s[4][2].tolist() == s[8][2].tolist() == [[1, 75 * 300 + 75, 75 * 300 + 75, 1]] and 75 * 300 + 75 > 22000
    assert by["comb_96x200"]["per"][4][2].tolist() == [[1, 100 * 95 + 200, 100 * 95 + 200, 1]]
    assert by["spiral_65x129"]["per"][4][2][0, 0] == by["spiral_65x129"]["per"][8][2][0, 0] == 2
    assert by["ring_blob_48x64"]["per"][8][2][0, 0] == 2
    assert min(by["noise_64x128"]["per"][4][2][0, 0], by["noise_60x107_thr03"]["per"][4][2][0, 0]) >= 100

    # the tracking sequence: expected outputs of the selection rule (8-connectivity)
    mask, lab = track["mask"], track["per"][8][0]
    first = obj[:1]
    settings = [("chain_r3", 1, radius, 0, 0, first, -np.inf), ("chain_r0", 1, 0, 0, 0, first, np.float32(-7.5)),
                ("frames_r3", 0, radius, 0, 0, obj, -np.inf), ("keep_largest", 1, radius, 0, 1, first, np.float32(-30.0)),
                ("min_area5", 1, radius, 5, 0, first, -np.inf)]
    kepts = {}
    for s, chain, r, min_area, keep_largest, seed, fill in settings:
        kept = select(mask, lab, seed, chain, r, min_area, keep_largest)
        assert not (kept & ~mask).any()
        kepts[s] = kept
        p = "track|%s|" % s
        out[p + "params"] = np.array([chain, r, min_area, keep_largest, 8], dtype=np.int64)
        out[p + "fill"] = np.float32(fill)
        out[p + "seed"] = cc.pack(seed)
        out[p + "kept"] = cc.pack(kept)
        out[p + "dropped"] = cc.pack(mask & ~kept)
        print("track %-13s kept pixels per frame %s" % (s, kept.reshape(8, -1).sum(1).tolist()))
    names = [s[0] for s in settings]
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert not np.array_equal(kepts[a], kepts[b]), (a, b)      # no flag can be silently ignored
    k = kepts["chain_r3"]
    distractor = np.zeros((48, 64), dtype=bool)
    distractor[6:13, 48:57] = True
    assert not k[4].any()                                              # the object is absent, the distractor is far from the last kept map
    assert not (k[2] & distractor).any() and not (k[3] & distractor).any()
    assert np.array_equal(k[5], mask[5])                               # an empty seed: everything passes
    assert (k[6] & distractor).sum() == distractor.sum()               # ... and the distractor then tracks itself: the documented behaviour
    assert not (kepts["frames_r3"][6] & distractor).any()
    out["track|settings"] = np.array(names)
    out["names"] = np.array([c["name"] for c in cases])
    path = os.path.join(HERE, "components.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("%s: %d bytes" % (path, size))
    assert size < 200 * 1024


if __name__ == "__main__":
    main()
