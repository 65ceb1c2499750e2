#!/usr/bin/env python3
"""Time the softmax readout of appearance matching (osvos_pytorch_amd.match.soft -> osvos_match_soft, csrc/match_soft.hip) next to
osvos_match_nearest of the same process, which it leaves unchanged and which is therefore the yardstick, at a bank of P, 2 P and 4 P rows,
without and with ``best``; next to topk at K = 4 and K = 16, whose per-score epilogues bracket it; and the whole matcher call with
soft_beta = 10 next to the default matcher and the plain forward.

    python tools/time_match_soft.py [--out profiles/match_soft_timing.txt] [--parent-lib PATH]          (needs the GPU)

``--parent-lib`` names a shared library built from the PARENT commit's csrc/match.hip (with csrc/errors.cpp): its osvos_match_nearest is
loaded into this process and timed against this tree's through the same ctypes path, window by window.  The file is untouched, so the two
must be level: the window ranges overlap, and the output says whether they do.

The windowing of tools/time_match.py: a seeded 854x480 frame, N = 1, conv4_3 (layer 9: 60 x 107 = 6420 pixels of 512 channels) of an
untrained network searched against the same frame's features, repeated to 2 P and 4 P rows, under a half-and-half labelling; all loops in one
process on one stream, alternating window by window; device events around PASSES back-to-back calls; median [min .. max] of WINDOWS windows.
There is no bar: the numbers are recorded, and the only claims made from them are ratios within this run.

It also reports how far lse is from the float64 restatement of tests/match_soft_cases.py, as a fraction of that file's bar, on its largest
case: the hardware exponential's measured error.

NOT measured: layer 6, batches above 1, hardware counters, any accuracy.
"""
import argparse
import ctypes as C
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tools"))
sys.path.insert(2, os.path.join(REPO, "tests"))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import networks.vgg_osvos as vo  # noqa: E402
from osvos_pytorch_amd import _lib, match  # noqa: E402
from osvos_pytorch_amd.augment import augment_frame  # noqa: E402
from time_match import H, PASSES, SLOW_PASSES, W, WARM, WINDOWS, scene, stats, window  # noqa: E402

LAYER = 9
BANKS = (1, 2, 4)
BETA = 10.0
TOPK_K4, TOPK_K16 = 1.20, 1.86          # profiles/match_ext_timing.txt: topk at K = 4 and K = 16, x nearest


def direct_nearest(lib, q, rinv, r, rinv_r, label, sim, ws):
    """osvos_match_nearest of ``lib`` through ctypes, the pointers made once -> a callable"""
    n, p, c = (int(v) for v in q.shape)
    fn = lib.osvos_match_nearest
    fn.restype, fn.argtypes = _lib.PROTOTYPES["osvos_match_nearest"]
    ptrs = [C.c_void_p(t.data_ptr()) for t in (q, rinv, r, rinv_r, label, sim)] + [None, C.c_void_p(ws.data_ptr())]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        rc = fn(*ptrs, n, int(r.shape[0]), p, int(r.shape[1]), c, stream)
        assert rc == 0, rc
    return call


def exp2_error():
    """-> lines: the largest |lse - restatement| as a fraction of the bar on tests/match_soft_cases.py's largest case"""
    import match_soft_cases as ms
    lines = []
    for beta in ms.SOFT_BETAS:
        p = ms.soft_problem(300, 2049, 1024, beta, n=2, nr=1)
        t = [torch.from_numpy(np.array(p[k])).cuda() for k in ("Q", "rinv_q", "R", "rinv_r", "label")]
        got = match.soft(*t, beta).cpu().numpy().astype(np.float64)
        diff = np.abs(got - p["lse"])
        lines.append("  (300, 2049, 1024) beta %4g: |lse - float64 restatement| largest %.3e, %.3f of the bar there" % (beta, diff.max(), (diff / ms.bar_of(p, beta)).max()))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--precision", default="fp32x3")
    ap.add_argument("--parent-lib", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    net = vo.OSVOS(pretrained=0).to(device)
    net.set_precision(args.precision)
    frame = scene().to(device)
    x = augment_frame(frame, None, False, None)[0][None]

    def image():
        return augment_frame(frame, None, False, None)[0][None]

    def forward():
        with torch.no_grad():
            net.forward(image())

    mask = torch.zeros((1, H, W), device=device, dtype=torch.uint8)
    mask[:, :, :W // 2] = 1
    feat = net.forward_features(x, LAYER)[1].clone()
    _, h, w, c = (int(v) for v in feat.shape)
    p = h * w
    q, rinv = match.quantize(feat)
    q, rinv = q.view(1, p, c), rinv.view(1, p)
    label = match.cell_labels(mask, match.stride_of(LAYER)).view(1, p)
    loops = [("854x480 one test forward (augment_frame identity + net.forward)", forward, SLOW_PASSES, 0)]
    banks = {}
    for m in BANKS:
        banks[m] = tuple(torch.cat([t] * m, dim=1).contiguous() for t in (q, rinv, label))
    index = {}
    for m in BANKS:
        r, rinv_r, lab = banks[m]
        ops = 2.0 * p * p * m * c
        wn = match.nearest_workspace(1, p, p * m, c, device)
        wsf = match.soft_workspace(1, p, p * m, c, device)
        index["nearest", m] = len(loops)
        loops.append(("nearest, Pr = %d P (%d x %d x %d), the unchanged kernel" % (m, p, p * m, c),
                      lambda r=r, rinv_r=rinv_r, lab=lab, wn=wn: match.nearest(q, rinv, r, rinv_r, lab, ws=wn), PASSES, ops))
        index["soft", m] = len(loops)
        loops.append(("soft beta %g without best, Pr = %d P" % (BETA, m),
                      lambda r=r, rinv_r=rinv_r, lab=lab, wsf=wsf: match.soft(q, rinv, r, rinv_r, lab, BETA, ws=wsf), PASSES, ops))
        index["soft+best", m] = len(loops)
        loops.append(("soft beta %g with best, Pr = %d P" % (BETA, m),
                      lambda r=r, rinv_r=rinv_r, lab=lab, wsf=wsf: match.soft(q, rinv, r, rinv_r, lab, BETA, ws=wsf, with_best=True), PASSES, ops))
    for k in (4, 16):
        wk = match.topk_workspace(1, p, p, c, k, device)
        index["topk", k] = len(loops)
        loops.append(("topk K = %d, Pr = P (the yardstick epilogue)" % k, lambda k=k, wk=wk: match.topk(q, rinv, q, rinv, label, k, ws=wk), PASSES, 2.0 * p * p * c))
    sim = torch.empty((1, 2, p), device=device, dtype=torch.float32)
    wd = match.nearest_workspace(1, p, p, c, device)
    index["direct"] = len(loops)
    loops.append(("nearest of this tree, direct ctypes call, Pr = P", direct_nearest(_lib.lib(), q, rinv, q, rinv, label, sim, wd), PASSES, 2.0 * p * p * c))
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        sim_p = torch.empty_like(sim)
        index["parent"] = len(loops)
        loops.append(("nearest of the parent commit's build, direct ctypes call, Pr = P", direct_nearest(parent, q, rinv, q, rinv, label, sim_p, wd), PASSES,
                      2.0 * p * p * c))
    default = match.AppearanceMatcher(net, LAYER, 4.0).set_reference(x, mask)
    softm = match.AppearanceMatcher(net, LAYER, 4.0, soft_beta=BETA).set_reference(x, mask)
    index["default"] = len(loops)
    loops.append(("854x480 AppearanceMatcher, defaults (forward_features + quantize + nearest + fuse)", lambda: default(image()), SLOW_PASSES, 0))
    index["softm"] = len(loops)
    loops.append(("854x480 AppearanceMatcher soft_beta=%g (soft in place of nearest)" % BETA, lambda: softm(image()), SLOW_PASSES, 0))
    for _ in range(WARM):
        for _, fn, _, _ in loops:
            fn()
    if args.parent_lib:
        torch.cuda.synchronize()
        assert torch.equal(sim.view(torch.int32), sim_p.view(torch.int32)), "the parent's nearest gives other bytes"
    times = [[] for _ in loops]
    for _ in range(WINDOWS):
        for i, (_, fn, passes, _) in enumerate(loops):
            times[i].append(window(fn, passes))
    med = [float(np.median(t)) for t in times]
    near = med[index["nearest", 1]]
    lines = ["command: python tools/time_match_soft.py%s   (%s, torch %s, precision %s, GPU_MAX_HW_QUEUES=%s)"
             % (" --parent-lib <the parent commit's csrc/match.hip>" if args.parent_lib else "", torch.cuda.get_device_name(0), torch.__version__,
                args.precision, os.environ.get("GPU_MAX_HW_QUEUES", "unset")),
             "batch 1, conv4_3 of an untrained network on a seeded 854x480 frame (P = %d rows of %d channels), searched against itself repeated to" % (p, c),
             "P, 2 P and 4 P rows under a half-and-half labelling; us per CALL through the Python wrapper (every launch of the call, output allocation",
             "included; the two 'direct' loops through ctypes alone), median [min .. max] of %d windows of %d calls (%d for the forward and the" % (WINDOWS, PASSES, SLOW_PASSES),
             "matchers), device events, the loops alternating in one process on one stream; 'x nearest' is the ratio of medians to nearest at Pr = P,",
             "'x same bank' to nearest at the same Pr, 'x forward' to the forward, all within this run; the int8 rate counts 2 multiply-adds per",
             "candidate pair and channel.  No bar is set: recorded, not gated.  Not measured: layer 6, batches above 1, hardware counters, any accuracy."]
    same = {}
    for key, i in index.items():
        if isinstance(key, tuple) and key[0] in ("nearest", "soft", "soft+best"):
            same[i] = med[index["nearest", key[1]]]
    for i, ((name, _, _, n_ops), t, m) in enumerate(zip(loops, times, med)):
        rate = "   %7.2f int8 Top/s" % (n_ops / (m * 1e-6) / 1e12) if n_ops else ""
        bank = "   x same bank %6.3f" % (m / same[i]) if i in same else ""
        lines.append("  %-92s %s   x nearest %6.3f   x forward %6.3f%s%s" % (name, stats(t), m / near, m / med[0], bank, rate))
    s1, sb1 = med[index["soft", 1]] / near, med[index["soft+best", 1]] / near
    k4, k16 = med[index["topk", 4]] / near, med[index["topk", 16]] / near
    lines.append("  the yardstick: topk costs %.3f x nearest at K = 4 and %.3f x at K = 16 in this run (%.2f and %.2f in profiles/match_ext_timing.txt); soft costs"
                 % (k4, k16, TOPK_K4, TOPK_K16))
    lines.append("  %.3f x without best and %.3f x with it: %s" % (s1, sb1, "inside the bracket or below it" if sb1 <= k16 else "ABOVE topk at K = 16"))
    lines.append("  default matcher minus forward: %.1f us; soft matcher minus default matcher: %.1f us (%.3f of the forward)"
                 % (med[index["default"]] - med[0], med[index["softm"]] - med[index["default"]], (med[index["softm"]] - med[index["default"]]) / med[0]))
    if args.parent_lib:
        a, b = times[index["direct"]], times[index["parent"]]
        level = min(a) <= max(b) and min(b) <= max(a)
        lines.append("  no regression of the untouched search: this tree %s, the parent's build %s -- the window ranges %s; the two give the same bytes"
                     % (stats(a).strip(), stats(b).strip(), "OVERLAP: level" if level else "DO NOT OVERLAP"))
    lines.append("the hardware exponential against the float64 restatement (tests/match_soft_cases.py; reported, the GPU tests gate it):")
    lines += exp2_error()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
