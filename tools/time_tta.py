#!/usr/bin/env python3
"""Time test-time augmentation (osvos_pytorch_amd.tta.TestTimeAugment: osvos_tta_view per view, one network forward per scale, one
osvos_tta_fuse) next to the plain test loop it replaces (osvos_augment_frame's identity pass + one forward), and the two kernels alone.

    python tools/time_tta.py [--out profiles/tta.txt]          (needs the GPU)

One seeded random uint8 854x480 frame through an untrained network (a forward's time does not depend on the weights), test precision as
train_online.py's default.  Configurations: scales (1,), (1,) + flip, (0.75, 1, 1.25) + flip.  All loops run in the same process on the
same frame, alternating window by window; device events around PASSES back-to-back calls (nothing waits for the host inside a window).
Median [min .. max] of WINDOWS windows, per FRAME.  The yardstick is the plain loop of the same run; the expectation from pixel counts is
the sum of s^2 forwards, twice that with flip.
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
from osvos_pytorch_amd import tta  # noqa: E402
from osvos_pytorch_amd.augment import augment_frame  # noqa: E402

PASSES, WARM, WINDOWS = 20, 3, 7
KERNEL_PASSES = 200


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--precision", default="fp32x3")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    device = torch.device("cuda:0")
    h, w = 480, 854
    torch.manual_seed(0)
    net = vo.OSVOS(pretrained=0).to(device)
    net.set_precision(args.precision)
    frame = torch.from_numpy(np.random.default_rng(0).integers(0, 256, size=(h, w, 3)).astype(np.uint8)).to(device)
    configs = [("scales (1,)", (1.0,), False), ("scales (1,) + flip", (1.0,), True), ("scales (0.75, 1, 1.25) + flip", (0.75, 1.0, 1.25), True)]
    state = {}

    def plain():
        with torch.no_grad():
            state["plain"] = net.forward(augment_frame(frame, None, False, None)[0][None])[-1]

    loops = [("plain loop: augment_frame (identity) + net.forward", plain, 1.0)]
    for name, scales, flip in configs:
        t = tta.TestTimeAugment(net.forward, scales, flip)

        def run(t=t, name=name):
            state[name] = t(frame)
        loops.append(("TestTimeAugment, " + name, run, sum(s * s for s in scales) * (2 if flip else 1)))
    for _ in range(WARM):
        for _, fn, _ in loops:
            fn()
    times = [[] for _ in loops]
    for _ in range(WINDOWS):
        for i, (_, fn, _) in enumerate(loops):
            times[i].append(window(fn, PASSES))
    same = bool(torch.equal(state["plain"], state[configs[0][0]]))
    base = np.median(times[0])
    lines = ["command: python tools/time_tta.py   (%s, torch %s, precision %s, GPU_MAX_HW_QUEUES=%s)"
             % (torch.cuda.get_device_name(0), torch.__version__, args.precision, os.environ.get("GPU_MAX_HW_QUEUES", "unset")),
             "one %dx%d uint8 frame, batch 1; us per FRAME, median [min .. max] of %d windows of %d calls, device events, the loops alternating in"
             % (w, h, WINDOWS, PASSES),
             "one process on one stream; 'x plain' is the ratio of medians to the plain loop of this run, 'pixels' the sum of s^2 (x 2 with flip)."]
    for (name, _, px), t in zip(loops, times):
        lines.append("  %-52s %s   x plain %5.2f   pixels %5.2f" % (name, stats(t), np.median(t) / base, px))
    lines.append("  TestTimeAugment with scales (1,) equals the plain loop bit for bit: %s" % same)
    assert same, "the single-scale TTA output differs from the plain forward"

    # the two kernels alone, at the sizes of the largest configuration
    lines.append("the kernels alone through their Python wrappers (back-to-back calls: the larger of the kernel time and the host's enqueue time),")
    lines.append("us per CALL, median [min .. max] of %d windows of %d calls.  '>= GB/s' = (bytes read once + bytes written) / median: a LOWER bound on" % (WINDOWS, KERNEL_PASSES))
    lines.append("the kernel's rate wherever the host's enqueue is the slower of the two (times flat across sizes say so), not its bandwidth:")
    f4 = frame[None]
    for s in (0.75, 1.0, 1.25):
        hv, wv = tta.view_size(h, w, s)
        out = torch.empty((1, 3, hv, wv), device=device, dtype=torch.float32)
        for flip in (False, True):
            fn = lambda: tta.make_view(f4, hv, wv, flip, out=out)  # noqa: E731
            fn()
            t = [window(fn, KERNEL_PASSES) for _ in range(WINDOWS)]
            nbytes = 3 * h * w + 12 * hv * wv
            lines.append("  osvos_tta_view %4dx%-4d%s %s   >= %6.0f GB/s" % (wv, hv, " mirrored" if flip else "         ", stats(t), nbytes / np.median(t) * 1e-3))
    gen = torch.Generator(device="cpu").manual_seed(1)
    for name, scales, flip in configs:
        p = tta.plan(h, w, scales, flip)
        maps = [(torch.rand(1, 1, hv, wv, generator=gen) * 40 - 20).to(device) for hv, wv, _ in p]
        out = torch.empty((1, 1, h, w), device=device, dtype=torch.float32)
        fn = lambda: tta.fuse_views(maps, [f for _, _, f in p], (h, w), out=out)  # noqa: E731
        fn()
        t = [window(fn, KERNEL_PASSES) for _ in range(WINDOWS)]
        nbytes = 4 * h * w + sum(4 * hv * wv for hv, wv, _ in p)
        lines.append("  osvos_tta_fuse V %d, %-30s %s   >= %6.0f GB/s" % (len(p), name, stats(t), nbytes / np.median(t) * 1e-3))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
