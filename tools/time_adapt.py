#!/usr/bin/env python3
"""Time online adaptation (osvos_pytorch_amd.adapt.OnlineAdapter) next to the plain test forward and the plain training micro-batch of the
same process, and its device pieces alone: osvos_mask_sqdist on a sparse mask and on a blob, osvos_adapt_targets.

    python tools/time_adapt.py [--out profiles/adapt.txt]          (needs the GPU)

One 854x480 frame, batch 1, an untrained network (the time of a step does not depend on the weights) whose fused bias is raised so that its
output is confident everywhere -- every frame has positive and negative targets and is adapted on, none is skipped.  The yardstick is the
micro-batch of the same run: an adapted frame should cost about `steps` micro-batches plus two forwards, and the targets a small fraction of
one micro-batch.  Loops alternate window by window; device events around back-to-back calls; median [min .. max] of WINDOWS windows.
"""
import argparse
import ctypes as C
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import networks.vgg_osvos as vo  # noqa: E402
from osvos_pytorch_amd import _lib, adapt  # noqa: E402
from osvos_pytorch_amd.train_common import TrainLoop, make_sgd  # noqa: E402

WARM, WINDOWS = 2, 5
KERNEL_PASSES = 100
STEPS, MIX = 15, 5


def window(fn, passes):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(passes):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / passes          # us per call


def stats(v, scale=1.0):
    return "%9.1f [%9.1f .. %9.1f]" % (np.median(v) * scale, min(v) * scale, max(v) * scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--precision", default="fp32x3")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    device = torch.device("cuda:0")
    h, w = 480, 854
    vp = C.c_void_p
    l = _lib.lib()
    stream = vp(torch.cuda.current_stream().cuda_stream)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    blob = ((((yy - 0.5 * h) / (0.25 * h)) ** 2 + ((xx - 0.5 * w) / (0.25 * w)) ** 2) <= 1).astype(np.uint8)
    sparse = np.zeros((h, w), dtype=np.uint8)
    sparse[h - 1, w - 1] = 1
    lines = ["command: python tools/time_adapt.py   (%s, torch %s, precision %s, GPU_MAX_HW_QUEUES=%s)"
             % (torch.cuda.get_device_name(0), torch.__version__, args.precision, os.environ.get("GPU_MAX_HW_QUEUES", "unset")),
             "one %dx%d frame, batch 1.  The kernels alone, straight through the C ABI on preallocated buffers: us per CALL, median [min .. max] of"
             % (w, h),
             "%d windows of %d back-to-back calls (device events)." % (WINDOWS, KERNEL_PASSES)]

    # the distance map: two launches (column pass, row pass)
    out = torch.empty((1, h, w), device=device, dtype=torch.int32)
    ws = torch.empty(int(l.osvos_adapt_ws_bytes(1, h, w)) // 4, device=device, dtype=torch.int32)
    sq = {}
    for name, host, invert in (("sparse: one pixel in the far corner (every walk runs its whole row)", sparse, 0),
                               ("empty: no source at all (the same walks, nothing found)", np.zeros_like(sparse), 0),
                               ("blob: the ellipse of the synthetic frame", blob, 0),
                               ("blob, inverted (distance to the background)", blob, 1)):
        m = torch.from_numpy(host).to(device)[None].contiguous()
        fn = lambda: _lib.check(l.osvos_mask_sqdist(vp(m.data_ptr()), invert, vp(out.data_ptr()), 1, h, w, vp(ws.data_ptr()), stream))  # noqa: E731
        fn()
        t = [window(fn, KERNEL_PASSES) for _ in range(WINDOWS)]
        sq[name] = np.median(t)
        lines.append("  osvos_mask_sqdist   %-70s %s" % (name, stats(t)))

    # the targets: two distance maps (four launches) and a 24-byte memset
    rng = np.random.RandomState(0)
    logits = torch.from_numpy((np.where(np.roll(blob, 40, axis=1) != 0, 4.0, -4.0) + 1.5 * rng.randn(h, w)).astype(np.float32)).to(device)[None]
    prev = torch.from_numpy(blob).to(device)[None].contiguous()
    label = torch.empty((1, h, w), device=device, dtype=torch.float32)
    counts = torch.empty((1, 3), device=device, dtype=torch.int64)
    t_targets = {}
    for erosion, distance in ((15, 220), (15, 40)):
        fn = lambda: _lib.check(l.osvos_adapt_targets(vp(logits.data_ptr()), vp(prev.data_ptr()), float(np.log(0.97 / 0.03)), erosion, distance,  # noqa: E731
                                                      vp(label.data_ptr()), vp(counts.data_ptr()), 1, h, w, vp(ws.data_ptr()), stream))
        fn()
        t = [window(fn, KERNEL_PASSES) for _ in range(WINDOWS)]
        t_targets[(erosion, distance)] = np.median(t)
        lines.append("  osvos_adapt_targets erosion %2d, distance %3d on the blob: (n_pos, n_neg, n_void) = %-26s %s"
                     % (erosion, distance, tuple(int(v) for v in counts[0].cpu().numpy()), stats(t)))

    # the loops
    torch.manual_seed(0)
    net = vo.OSVOS(pretrained=0).to(device)
    net.set_precision(args.precision)
    with torch.no_grad():
        net.fuse.bias.fill_(5.0)                     # confident everywhere: positives wherever the distance rule allows them
    image = (torch.randn(1, 3, h, w, generator=torch.Generator().manual_seed(1)) * 40.0).to(device)
    gt = torch.from_numpy(blob.astype(np.float32)).to(device)[None, None]
    plain_loop = TrainLoop(net, make_sgd(net, 'online'), mode='online', n_ave_grad=1)
    adapter = adapt.OnlineAdapter(net, make_sgd(net, 'online'), lambda: (image, gt), steps=STEPS, mix=MIX)

    def forward():
        with torch.no_grad():
            net.forward(image)

    def micro_batch():
        plain_loop.micro_batch(image, gt)

    def adapted():
        adapter(image, prev)

    def targets_wrapped():
        adapt.adaptation_targets(logits, prev)

    loops = [("plain test forward (no_grad net.forward)", forward, 10), ("plain TrainLoop.micro_batch, one optimizer step each", micro_batch, 10),
             ("adaptation_targets through the Python wrapper (allocates)", targets_wrapped, 10),
             ("OnlineAdapter, steps %d, mix %d: per FRAME" % (STEPS, MIX), adapted, 3)]
    for _ in range(WARM):
        for _, fn, _ in loops:
            fn()
    times = [[] for _ in loops]
    for _ in range(WINDOWS):
        for i, (_, fn, passes) in enumerate(loops):
            times[i].append(window(fn, passes))
    s = adapter.summary()
    assert s["skipped"] == 0, "the timed frames were skipped: %r" % (s,)
    t_fwd, t_mb, t_tw, t_ad = (np.median(t) for t in times)
    lines.append("the loops, in one process on one stream, alternating window by window: ms per call, median [min .. max] of %d windows" % WINDOWS)
    for (name, _, passes), t in zip(loops, times):
        lines.append("  %-66s %s   (%d calls per window)" % (name, stats(t, 1e-3), passes))
    lines.append("  adapted frames %d, skipped %d, optimizer steps %d" % (s["adapted"], s["skipped"], s["steps"]))
    lines.append("an adapted frame costs %.1f micro-batches of this run (%d steps + 2 forwards + targets = %.1f expected from the parts);"
                 % (t_ad / t_mb, STEPS, (STEPS * t_mb + 2 * t_fwd + t_tw) / t_mb))
    worst = max(t_targets.values())
    lines.append("osvos_adapt_targets costs %.3f of one micro-batch (%.0f us of %.0f us); the worst distance map (%.0f us) %.3f of one."
                 % (worst / t_mb, worst, t_mb, max(sq.values()), max(sq.values()) / t_mb))
    lines.append("targets cost MORE than one micro-batch: revisit the row pass" if worst > t_mb else
                 "targets cost less than one micro-batch: the outward-walk row pass stays")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
