"""Shared by the connected-component tests and tests/golden/make_components_golden.py: reads tests/golden/components.npz and turns a case
into the logits a test feeds to the device.  Nothing here labels a component, measures an area or applies the selection rule.

Fixture layout (one entry per case name in ``names``; masks are bit-packed with np.packbits over the flattened [N, H, W] array):
    <name>|meta      int64 [3]           N, H, W
    <name>|thr       float64             probability threshold (0.5 unless the case says otherwise)
    <name>|mask      uint8 packed        the foreground P of every frame
    <name>|special   int64 [M, 4]        rows (n, y, x, kind): BACKGROUND pixels whose logit ``logits`` sets by hand, see the kinds below
    <name>|labels4   int32 [N, H, W]     canonical labels under 4-connectivity: 0 off P, else 1 + the lowest flat index of the component
    <name>|area4     int32 [N, H, W]     the component's pixel count at its root pixel, 0 elsewhere
    <name>|stats4    int64 [N, 4]        components, |P|, largest area, label of the largest (lowest label on a tie, 0 when there is none)
    <name>|labels8, |area8, |stats8      the same under 8-connectivity; left out when equal to the 4-connectivity arrays
The tracking sequence ``track`` also has, per setting s in ``track|settings``:
    track|<s>|params   int64 [5]         chain, seed radius, min_area, keep_largest, connectivity
    track|<s>|fill     float32           what dropped pixels receive
    track|<s>|seed     uint8 packed      the seed maps: [1, H, W] when chain, else [N, H, W]
    track|<s>|kept     uint8 packed      expected kept maps [N, H, W]
    track|<s>|dropped  uint8 packed      the pixels at which the filtered logits hold `fill`; everywhere else they equal the input.  (The
                                         filtered logits of ``logits(case)`` are stored in this exact form -- ``expected_out`` rebuilds them --
                                         because forty frames of random floats do not compress.)
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "components.npz")
# kinds of special pixels (both are background)
THR_EQ = 1     # the logit EQUALS the logit threshold
NAN = 2        # the logit is NaN


def pack(a):
    return np.packbits(np.asarray(a, dtype=bool).reshape(-1))


def unpack(bits, shape):
    n = int(np.prod(shape))
    return np.unpackbits(bits)[:n].reshape(shape).astype(bool)


def load(path=GOLDEN):
    z = np.load(path)
    cases = []
    for name in [str(s) for s in z["names"]]:
        n, h, w = [int(v) for v in z[name + "|meta"]]
        c = {"name": name, "N": n, "H": h, "W": w, "thr": float(z[name + "|thr"]), "mask": unpack(z[name + "|mask"], (n, h, w)),
             "special": z[name + "|special"].astype(np.int64).reshape(-1, 4)}
        for key in ("labels", "area", "stats"):
            c[key] = {4: z["%s|%s4" % (name, key)]}
            c[key][8] = z["%s|%s8" % (name, key)] if "%s|%s8" % (name, key) in z.files else c[key][4]
        if name + "|settings" in z.files:
            c["settings"] = {}
            for s in [str(v) for v in z[name + "|settings"]]:
                p = "%s|%s|" % (name, s)
                chain, radius, min_area, keep_largest, conn = [int(v) for v in z[p + "params"]]
                c["settings"][s] = {"chain": chain, "radius": radius, "min_area": min_area, "keep_largest": keep_largest, "conn": conn,
                                    "fill": float(z[p + "fill"]), "seed": unpack(z[p + "seed"], (1 if chain else n, h, w)),
                                    "kept": unpack(z[p + "kept"], (n, h, w)), "dropped": unpack(z[p + "dropped"], (n, h, w))}
        cases.append(c)
    return cases


def logit_threshold(thr):
    return np.float32(np.log(thr / (1.0 - thr)))


def logits(case, seed=0):
    """float32 [N, H, W] whose thresholded mask is the case's ``mask``: foreground sits above the logit threshold t by 1e-3 .. ~8, background
    below it by 1e-3 .. ~6.  Then the special pixels are set by hand (see the kinds)."""
    rng = np.random.default_rng(3000 + seed)
    m, t = case["mask"], logit_threshold(case["thr"])
    above = (t + np.float32(1e-3) + (8.0 * rng.random(m.shape) ** 3).astype(np.float32)).astype(np.float32)
    below = (t - np.float32(1e-3) - (6.0 * rng.random(m.shape) ** 2).astype(np.float32)).astype(np.float32)
    x = np.where(m, above, below).astype(np.float32)
    for n, y, xx, kind in case["special"]:
        if kind == THR_EQ:
            x[n, y, xx] = t
        elif kind == NAN:
            x[n, y, xx] = np.nan
        else:
            raise ValueError("special pixel kind %d" % kind)
    return x


def expected_out(setting, x):
    """the filtered logits of input x under a stored setting: `fill` at the stored dropped pixels, x everywhere else"""
    return np.where(setting["dropped"], np.float32(setting["fill"]), x).astype(np.float32)
