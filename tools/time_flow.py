#!/usr/bin/env python3
"""Time the motion compensation (osvos_pytorch_amd.flow -> osvos_flow_block_match / osvos_flow_warp, csrc/flow.hip) next to one test forward
of the network, the step it runs in front of.

    python tools/time_flow.py [--out profiles/flow_timing.txt]          (needs the GPU)

A seeded 854x480 noise frame and the same frame displaced by (17, -9), N = 1; the default parameters (search 24, block 16, step 4, penalty
4, median 1) and the same with search 48.  All loops run in one process on one stream, alternating window by window; device events around
PASSES back-to-back calls (nothing waits for the host inside a window).  Median [min .. max] of WINDOWS windows.  The forward runs an
untrained network (a forward's time does not depend on the weights) at train_online.py's default test precision.  There is no bar: the
numbers are recorded, and the only claim made from them is the ratio to the forward of the same run.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import networks.vgg_osvos as vo  # noqa: E402
from osvos_pytorch_amd import flow  # noqa: E402
from osvos_pytorch_amd.augment import augment_frame  # noqa: E402

PASSES, WARM, WINDOWS = 20, 3, 7
SLOW_PASSES = 5          # the forward: milliseconds per call
H, W, SHIFT = 480, 854, (17, -9)


def window(fn, passes):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(passes):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / passes          # us per call


def stats(v):
    return "%9.1f [%9.1f .. %9.1f]" % (np.median(v), min(v), max(v))


def scene(seed=0):
    """(prev, cur) uint8 [1,H,W,3] with cur(p) = prev(p + SHIFT) inside the frame"""
    dx, dy = SHIFT
    m = max(abs(dx), abs(dy))
    big = np.random.default_rng(seed).integers(0, 256, size=(H + 2 * m, W + 2 * m, 3), dtype=np.uint8)
    return (torch.from_numpy(big[None, m:m + H, m:m + W].copy()), torch.from_numpy(big[None, m + dy:m + dy + H, m + dx:m + dx + W].copy()))


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
    prev, cur = [t.to(device) for t in scene()]
    mask = (torch.rand(1, H, W, device=device) > 0.5).to(torch.uint8)
    state = {}

    def forward():
        with torch.no_grad():
            state["fwd"] = net.forward(augment_frame(cur[0], None, False, None)[0][None])[-1]
    loops = [("854x480 one test forward (augment_frame identity + net.forward)", forward, SLOW_PASSES)]
    for search in (24, 48):
        kw = dict(search=search, block=16, step=4, penalty=4, median=1)
        ws = flow.workspace(1, H, W, kw["block"], kw["step"], search, kw["median"], device)
        vec, cost = flow.block_match(prev, cur, ws=ws, **kw)
        inner = vec[0, 10:-10, 10:-10].reshape(-1, 2)
        exact = float((inner == torch.tensor(SHIFT, device=device, dtype=torch.int32)).all(-1).float().mean())
        assert exact == 1.0, "the matcher does not return the displacement of the scene: %g" % exact
        tag = "854x480 search %2d block 16 step 4 median 1 (%4d candidates)" % (search, (2 * search + 1) ** 2)
        loops.append((tag + " block_match", lambda kw=kw, ws=ws: flow.block_match(prev, cur, ws=ws, **kw), PASSES))
        if search == 24:
            loops.append(("854x480 warp of a uint8 mask along that field", lambda vec=vec: flow.warp(mask, vec, 4), PASSES))
    for _ in range(WARM):
        for _, fn, _ in loops:
            fn()
    times = [[] for _ in loops]
    for _ in range(WINDOWS):
        for i, (_, fn, passes) in enumerate(loops):
            times[i].append(window(fn, passes))
    lines = ["command: python tools/time_flow.py   (%s, torch %s, precision %s, GPU_MAX_HW_QUEUES=%s)"
             % (torch.cuda.get_device_name(0), torch.__version__, args.precision, os.environ.get("GPU_MAX_HW_QUEUES", "unset")),
             "batch 1, a noise frame against itself displaced by (%d, %d); us per CALL through the Python wrapper (luma, matcher and median launches," % SHIFT,
             "output allocation included), median [min .. max] of %d windows of %d calls (%d for the forward), device events, the loops alternating"
             % (WINDOWS, PASSES, SLOW_PASSES),
             "in one process on one stream; 'x forward' is the ratio of medians to the forward of this run.  No bar is set: recorded, not gated."]
    fwd = float(np.median(times[0]))
    for (name, _, _), t in zip(loops, times):
        lines.append("  %-78s %s   x forward %6.3f" % (name, stats(t), np.median(t) / fwd))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
