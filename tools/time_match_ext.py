#!/usr/bin/env python3
"""Time the two searches added to appearance matching (osvos_pytorch_amd.match.topk / local -> osvos_match_topk / osvos_match_local,
csrc/match_ext.hip) next to osvos_match_nearest of the same process, which they leave unchanged and which is therefore the yardstick, and
the whole matcher call with both options next to the default matcher and the plain forward.

    python tools/time_match_ext.py [--out profiles/match_ext_timing.txt]          (needs the GPU)

The windowing of tools/time_match.py: a seeded 854x480 frame, N = 1, conv4_3 (layer 9: 60 x 107 = 6420 pixels of 512 channels) of an
untrained network searched against the same frame's features under a half-and-half labelling; all loops in one process on one stream,
alternating window by window; device events around PASSES back-to-back calls; median [min .. max] of WINDOWS windows.  There is no bar: the
numbers are recorded, and the only claims made from them are ratios within this run.

NOT measured: batches above 1, layer 6, hardware counters.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tools"))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import networks.vgg_osvos as vo  # noqa: E402
from osvos_pytorch_amd import match  # noqa: E402
from osvos_pytorch_amd.augment import augment_frame  # noqa: E402
from time_match import H, PASSES, SLOW_PASSES, W, WARM, WINDOWS, scene, stats, window  # noqa: E402

LAYER = 9
KS = (1, 4, 8, 16)
RADII = (2, 4, 8)
MATCHER = dict(topk=4, local_radius=4, local_gain=2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--precision", default="fp32x3")
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
    ops = 2.0 * p * p * c
    ws = match.nearest_workspace(1, p, p, c, device)
    loops = [("854x480 one test forward (augment_frame identity + net.forward)", forward, SLOW_PASSES, 0),
             ("nearest (%d x %d x %d), the unchanged kernel" % (p, p, c), lambda: match.nearest(q, rinv, q, rinv, label, ws=ws), PASSES, ops)]
    for k in KS:
        wk = match.topk_workspace(1, p, p, c, k, device)
        loops.append(("topk K = %d (list length %d)" % (k, 4 if k <= 4 else 8 if k <= 8 else 16),
                      lambda k=k, wk=wk: match.topk(q, rinv, q, rinv, label, k, ws=wk), PASSES, ops))
    for radius in RADII:
        cells = sum(min(i + radius, h - 1) - max(i - radius, 0) + 1 for i in range(h)) * sum(min(j + radius, w - 1) - max(j - radius, 0) + 1 for j in range(w))
        loops.append(("local radius %d (%d x %d grid, %d candidate pairs)" % (radius, h, w, cells),
                      lambda radius=radius: match.local(q, rinv, q, rinv, label, grid=(h, w), radius=radius), PASSES, 2.0 * cells * c))
    default = match.AppearanceMatcher(net, LAYER, 4.0).set_reference(x, mask)
    both = match.AppearanceMatcher(net, LAYER, 4.0, **MATCHER).set_reference(x, mask)
    both(image(), None)                          # the local view needs a previous call
    loops.append(("854x480 AppearanceMatcher, defaults (forward_features + quantize + nearest + fuse)", lambda: default(image()), SLOW_PASSES, 0))
    loops.append(("854x480 AppearanceMatcher topk=%d local_radius=%d (+ cell_labels + local, three views fused)" % (MATCHER["topk"], MATCHER["local_radius"]),
                  lambda: both(image(), mask), SLOW_PASSES, 0))
    for _ in range(WARM):
        for _, fn, _, _ in loops:
            fn()
    times = [[] for _ in loops]
    for _ in range(WINDOWS):
        for i, (_, fn, passes, _) in enumerate(loops):
            times[i].append(window(fn, passes))
    med = [float(np.median(t)) for t in times]
    lines = ["command: python tools/time_match_ext.py   (%s, torch %s, precision %s, GPU_MAX_HW_QUEUES=%s)"
             % (torch.cuda.get_device_name(0), torch.__version__, args.precision, os.environ.get("GPU_MAX_HW_QUEUES", "unset")),
             "batch 1, conv4_3 of an untrained network on a seeded 854x480 frame, searched against itself under a half-and-half labelling; us per CALL",
             "through the Python wrapper (every launch of the call, output allocation included), median [min .. max] of %d windows of %d calls (%d for"
             % (WINDOWS, PASSES, SLOW_PASSES),
             "the forward and the matchers), device events, the loops alternating in one process on one stream; 'x nearest' and 'x forward' are ratios",
             "of medians within this run; the int8 rate counts 2 multiply-adds per candidate pair and channel.  No bar is set: recorded, not gated.",
             "Not measured: batches above 1, layer 6, hardware counters."]
    for (name, _, _, n_ops), t, m in zip(loops, times, med):
        rate = "   %7.2f int8 Top/s" % (n_ops / (m * 1e-6) / 1e12) if n_ops else ""
        lines.append("  %-100s %s   x nearest %6.3f   x forward %6.3f%s" % (name, stats(t), m / med[1], m / med[0], rate))
    lines.append("  default matcher minus forward: %.1f us; matcher with both options minus default matcher: %.1f us (%.3f of the forward)"
                 % (med[-2] - med[0], med[-1] - med[-2], (med[-1] - med[-2]) / med[0]))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
