#!/usr/bin/env python3
"""A/B of precisions 'bf16', 'bf16w2' and 'fp32x3' in ONE process on one GPU: the configs[2] loop (parent mode, 854x480, batch 12, five losses,
FusedSGD, TrainLoop -- train_parent.py:132-172) timed with hip events, the precisions alternating over several rounds; then a per-layer table of the
forward convolutions at batch 12: the single-piece bf16 launch against the two-piece ('bf16w2') one, automatic tile and every two-piece tile forced.
Prints a text report (profiles/bf16w2_ab.txt is one)."""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ap = argparse.ArgumentParser()
ap.add_argument("--precisions", default="bf16,bf16w2,fp32x3")
ap.add_argument("--batch", type=int, default=12)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--width", type=int, default=854)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--steps", type=int, default=50, help="micro-batches timed per precision and round")
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--layer-reps", type=int, default=20)
ap.add_argument("--no-loop", action="store_true")
ap.add_argument("--no-layers", action="store_true")
args = ap.parse_args()

from bench import synth_problem  # noqa: E402  (the benchmark's seeded problem: He-init weights, calibrated heads)
from osvos_pytorch_amd import ops  # noqa: E402
from osvos_pytorch_amd._lib import BF16_W2, F32_BF16MFMA  # noqa: E402
from osvos_pytorch_amd.train_common import TrainLoop, make_sgd  # noqa: E402

dev = torch.device("cuda:0")
print("device: %s, torch %s, hip %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip))
print("configs[2] loop: parent mode, %dx%d, batch %d, nAveGrad 10, five losses, FusedSGD, TrainLoop; %d warm-up + %d timed micro-batches per "
      "precision and round, %d rounds, order rotated every round" % (args.width, args.height, args.batch, args.warmup, args.steps, args.rounds))


def ev_time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


if not args.no_loop:
    precs = args.precisions.split(",")
    runs = {}
    for p in precs:
        net, x, gt = synth_problem(args.batch, args.height, args.width, dev, seed=0)
        net.set_precision(p)
        loop = TrainLoop(net, make_sgd(net, "parent"), mode="parent", n_ave_grad=10)

        def step(loop=loop, x=x, gt=gt):
            loop.micro_batch(x.detach().requires_grad_(), gt, epoch=0)
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        runs[p] = step
    fps = {p: [] for p in precs}
    for r in range(args.rounds):
        order = precs[r % len(precs):] + precs[:r % len(precs)]
        for p in order:
            runs[p]()              # (re-enter the precision's working set)
            torch.cuda.synchronize()
            ms = ev_time(runs[p], args.steps)
            fps[p].append(1000.0 * args.batch / ms)
            print("round %d %-7s %7.2f ms per micro-batch  %8.1f frames/s" % (r, p, ms, fps[p][-1]))
    print()
    base = max(fps["bf16"]) if "bf16" in fps else None
    for p in precs:
        best = max(fps[p])
        print("%-7s frames/s best %8.1f  all %s%s" % (p, best, " ".join("%.1f" % v for v in fps[p]),
                                                     ("   step time vs bf16 %+.1f %%" % (100.0 * (base / best - 1.0))) if base else ""))
    del runs
    torch.cuda.empty_cache()

if not args.no_layers:
    print()
    print("forward convolutions at batch %d (%dx%d), op level: bf16 in / bf16 out, ReLU (side_prep: none), no fused pool; ms per call, output "
          "zero-fill included (%d reps); bf16 / bf16w2 = automatic tile, tNN = two-piece tile NN forced"
          % (args.batch, args.width, args.height, args.layer_reps))
    chans = [[64, 64], [128, 128], [256, 256, 256], [512, 512, 512], [512, 512, 512]]
    layers = []
    h, w, cin = args.height, args.width, 8
    for si, st in enumerate(chans):
        if si > 0:
            h, w = (h + 1) // 2, (w + 1) // 2
        for j, c in enumerate(st):
            layers.append(("conv%d_%d" % (si + 1, j + 1), h, w, cin, c, cin if cin != 8 else 3))
            cin = c
        if si > 0:
            layers.append(("side_prep%d" % si, h, w, cin, 16, cin))
    w2_tiles = ops.conv3x3_bf16w2_tiles() + [142]      # (142: tile 42 with the XCD-local block order)
    print("%-11s %4s %4s %4s %4s | %8s | %8s %6s | %s" % ("layer", "h", "w", "cin", "cout", "bf16", "bf16w2", "ratio",
                                                         "  ".join("t%-6d" % t for t in w2_tiles)))
    tot1 = tot2 = 0.0
    g = torch.Generator().manual_seed(0)
    for name, h, w, cs, cout, cin_real in layers:
        x = torch.randn(args.batch, h, w, cs, generator=g).to(dev).bfloat16()
        if cs == 8:
            x[..., 3:] = 0
        wt = (torch.randn(cout, cin_real, 3, 3, generator=g) * (2.0 / (9 * cin_real)) ** 0.5).to(dev)
        b = torch.zeros(cout, device=dev)
        pk1, pk2 = ops.pack_fwd(wt, F32_BF16MFMA), ops.pack_fwd(wt, F32_BF16MFMA | BF16_W2)
        relu = not name.startswith("side")
        t1 = ev_time(lambda: ops.conv3x3_bf16act_fused(x, pk1, b, cout, relu=relu), 2)
        t1 = ev_time(lambda: ops.conv3x3_bf16act_fused(x, pk1, b, cout, relu=relu), args.layer_reps)
        t2 = ev_time(lambda: ops.conv3x3_bf16w2_fused(x, pk2, b, cout, relu=relu), 2)
        t2 = ev_time(lambda: ops.conv3x3_bf16w2_fused(x, pk2, b, cout, relu=relu), args.layer_reps)
        forced = []
        for t in w2_tiles:
            ev_time(lambda: ops.conv3x3_bf16w2_fused(x, pk2, b, cout, relu=relu, tile=t), 2)
            forced.append(ev_time(lambda: ops.conv3x3_bf16w2_fused(x, pk2, b, cout, relu=relu, tile=t), max(3, args.layer_reps // 4)))
        tot1 += t1
        tot2 += t2
        print("%-11s %4d %4d %4d %4d | %8.3f | %8.3f %6.2f | %s" % (name, h, w, cin_real, cout, t1, t2, t2 / t1, "  ".join("%7.3f" % v for v in forced)))
        del x, pk1, pk2
    print("%-11s %24s | %8.3f | %8.3f %6.2f |" % ("sum", "", tot1, tot2, tot2 / tot1))
