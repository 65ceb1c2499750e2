#!/usr/bin/env python3
"""Time the object-centred zoom (osvos_pytorch_amd.roi -> osvos_roi_box / osvos_roi_view / osvos_roi_paste, csrc/roi.hip) next to its
yardsticks in the same process: the test-time augmentation kernels that move the same bytes (osvos_tta_view and osvos_tta_fuse with one
view, at the same sizes; and osvos_tta_view of the box's window cut out beforehand, which is the crop view's arithmetic tap for tap), a
single torch pass over the same mask (torch.any), and one plain test forward, the step the zoom wraps.

    python tools/time_roi.py [--out profiles/roi_timing.txt]          (needs the GPU)

A seeded 854x480 frame, N = 1, canvas = the frame's size, max_zoom 2, margins (25, 8), the previous mask an ellipse over about 5 % of the
frame.  All loops run in one process on one stream, alternating window by window; device events around PASSES back-to-back calls (nothing
waits for the host inside a window).  Median [min .. max] of WINDOWS windows, in us per call = per frame.  Every call goes through its Python
wrapper with the output allocated by the call, the zoom's and the yardsticks' alike, so a kernel of a few microseconds is timed at the rate
the host can enqueue it: the window ranges say whether two such calls can be told apart at all.  The forward runs at train_online.py's
default test precision on an untrained network (a kernel's time does not depend on the values).  There is no bar: the numbers are recorded,
and the only claims made from them are the ratios to the forward of the same run.
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
from osvos_pytorch_amd import roi, tta  # noqa: E402
from osvos_pytorch_amd.augment import augment_frame  # noqa: E402

PASSES, WARM, WINDOWS = 50, 3, 7
SLOW_PASSES = 5          # the forward and the whole zoom: milliseconds per call
H, W = 480, 854


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
    """uint8 [H,W,3]: a few flat regions with curved borders under +-12 colour noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    region = ((xx - 300) ** 2 + (yy - 200) ** 2 < 150 ** 2).astype(int) + (np.sin(xx / 40.0) * 60 + 300 < yy).astype(int)
    pal = np.array([(120, 130, 60), (40, 90, 200), (200, 60, 90)])
    return torch.from_numpy(np.clip(pal[region] + rng.integers(-12, 13, size=(H, W, 3)), 0, 255).astype(np.uint8))


def ellipse(cx=500, cy=260, a=95, b=69):
    """bool [1,1,H,W]: about 5 % of the frame"""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return torch.from_numpy((((xx - cx) / float(a)) ** 2 + ((yy - cy) / float(b)) ** 2 <= 1.0)[None, None])


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
    frames = frame[None].contiguous()
    mask = ellipse().to(device)
    share = float(mask.float().mean())
    zoom = roi.RoiZoom(net.forward)
    box = roi.mask_box(mask, (H, W))
    logits = torch.randn((1, 1, H, W), device=device)
    bx = [int(v) for v in box.cpu().numpy()[0]]
    cropped = frames[:, bx[1]:bx[1] + bx[3], bx[0]:bx[0] + bx[2]].contiguous()          # the box's window as a frame of its own (made once, outside the loops)
    state = {}

    def forward():
        with torch.no_grad():
            state["fwd"] = net.forward(augment_frame(frame, None, False, None)[0][None])[-1]

    loops = [("one test forward (augment_frame identity + net.forward)", forward, SLOW_PASSES),
             ("RoiZoom whole (box + view + net.forward + paste)", lambda: zoom(frame, mask), SLOW_PASSES),
             ("osvos_roi_box (roi.mask_box: reads the %d KB mask; two launches)" % (H * W // 1000), lambda: roi.mask_box(mask, (H, W)), PASSES),
             ("torch.any over the same mask (one pass, one read)", lambda: torch.any(mask), PASSES),
             ("osvos_roi_view (roi.crop_view: the box's window -> 3 x 480 x 854 fp32)", lambda: roi.crop_view(frames, box, (H, W)), PASSES),
             ("osvos_tta_view (tta.make_view: the frame -> the same size)", lambda: tta.make_view(frames, H, W), PASSES),
             ("osvos_roi_paste (roi.paste: 480 x 854 fp32 -> the box, -20 elsewhere)", lambda: roi.paste(logits, box, (H, W)), PASSES),
             ("osvos_tta_fuse, one view (tta.fuse_views: 480 x 854 fp32 -> the same size)", lambda: tta.fuse_views([logits], [False], (H, W)), PASSES),
             ("osvos_tta_view of the box's window cut out beforehand (the same taps as roi_view)", lambda: tta.make_view(cropped, H, W), PASSES)]
    for _ in range(WARM):
        for _, fn, _ in loops:
            fn()
    times = [[] for _ in loops]
    for _ in range(WINDOWS):
        for i, (_, fn, passes) in enumerate(loops):
            times[i].append(window(fn, passes))
    lines = ["command: python tools/time_roi.py   (%s, torch %s, precision %s, GPU_MAX_HW_QUEUES=%s)"
             % (torch.cuda.get_device_name(0), torch.__version__, args.precision, os.environ.get("GPU_MAX_HW_QUEUES", "unset")),
             "854x480, batch 1, canvas = the frame's size, max_zoom 2, margins (25, 8); the previous mask an ellipse over %.1f %% of the frame, its box"
             % (100.0 * share),
             "(x0, y0, bw, bh) = %s: %.1f %% of the frame, enlarged %.2f times.  us per CALL = per frame, through the Python wrapper (every launch of the"
             % (tuple(bx), 100.0 * bx[2] * bx[3] / (H * W), W / float(bx[2])),
             "call, output allocation included), median [min .. max] of %d windows of %d calls (%d for the forward and the whole zoom), device events,"
             % (WINDOWS, PASSES, SLOW_PASSES),
             "the loops alternating in one process on one stream; 'x forward' is the ratio of medians to the forward of this run.  No bar is set:",
             "recorded, not gated."]
    med = [float(np.median(t)) for t in times]
    for (name, _, _), t in zip(loops, times):
        lines.append("  %-82s %s   x forward %7.4f" % (name, stats(t), np.median(t) / med[0]))
    lines.append("  zoom minus forward: %.1f us (%.4f of the forward); box + view + paste alone: %.1f us (%.4f of the forward)"
                 % (med[1] - med[0], (med[1] - med[0]) / med[0], med[2] + med[4] + med[6], (med[2] + med[4] + med[6]) / med[0]))

    def overlap(i, j):
        return max(min(times[i]), min(times[j])) <= min(max(times[i]), max(times[j]))

    def word(i, j):
        return "overlap" if overlap(i, j) else "do NOT overlap"
    lines.append("  window ranges: roi_view and the same-size tta_view %s, roi_view and tta_view of the cut-out window %s; roi_paste and tta_fuse %s;"
                 % (word(4, 5), word(4, 8), word(6, 7)))
    lines.append("  roi_box is %.2f times torch.any" % (med[2] / med[3]))
    lines.append("  (the view kernels all write the same 4.9 MB.  The same-size tta_view is that kernel's cheapest case: every tap falls on a sample, so the")
    lines.append("  second source row is never loaded and no product is formed; an enlarging view loads both rows and both columns of every pixel, and")
    lines.append("  the tta_view of the cut-out window is roi_view's arithmetic tap for tap.  The paste samples only the pixels of the box -- %.1f %% of"
                 % (100.0 * bx[2] * bx[3] / (H * W)))
    lines.append("  the frame here -- and stores a constant everywhere else, where the one-view fuse samples every pixel: the paste can be the faster of")
    lines.append("  the two.  The whole zoom runs the forward on another input, the enlarged crop, without the augment_frame call of the")
    lines.append("  plain test forward: its difference to the forward is the difference of two forwards, not the cost of the three kernels, which is the")
    lines.append("  sum above.)")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
