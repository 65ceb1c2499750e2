#!/usr/bin/env python3
"""Time the mask refinement (osvos_pytorch_amd.refine.CrfRefiner -> osvos_crf_refine, csrc/crf.hip: one launch per mean-field iteration)
next to (a) a plain torch implementation of the same rule (F.unfold gathers the window, fp32, on the same device) and (b) one test forward
of the network, the step whose output it refines.

    python tools/time_crf.py [--out profiles/crf_timing.txt]          (needs the GPU)

Seeded frames and logits of tests/crf_cases.scene's kind at 854x480 and 1920x1080, windows (radius, dilation) = (5, 3) and (3, 2), the
default weights and thetas.  All loops run in one process on one stream, alternating window by window; device events around PASSES
back-to-back calls (nothing waits for the host inside a window).  Median [min .. max] of WINDOWS windows.  'per iteration' is a
one-iteration call, 'five iterations' the default call; a 1x1 frame gives the cost of a launch through the wrapper.  The forward runs an
untrained network (a forward's time does not depend on the weights) at train_online.py's default test precision.
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
from osvos_pytorch_amd import refine  # noqa: E402
from osvos_pytorch_amd.augment import augment_frame  # noqa: E402

PASSES, WARM, WINDOWS = 50, 3, 7
SLOW_PASSES = 5          # the torch formulation and the forward: milliseconds per call


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


def scene(h, w, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    inside = ((yy - 0.5 * h) / (0.3 * h)) ** 2 + ((xx - 0.45 * w) / (0.3 * w)) ** 2 <= 1.0
    u = (np.where(inside, 2.0, -2.0) + rng.normal(0.0, 3.0, size=(h, w))).astype(np.float32)
    base = np.where(inside[..., None], np.array([40, 160, 220]), np.array([200, 90, 30]))
    fr = np.clip(base + rng.integers(-20, 21, size=(h, w, 3)), 0, 255).astype(np.uint8)
    return torch.from_numpy(u)[None], torch.from_numpy(fr)[None]


def torch_rule(u, fr, coeffs, iters, R, D):
    """the rule of include/osvos_hip.h in plain torch fp32: u [1,H,W], fr [1,H,W,3] uint8 -> [1,H,W]"""
    F = torch.nn.functional
    w_a, w_s, a_s, a_c, g_s = coeffs
    _, H, W = u.shape
    K = 2 * R + 1
    kw = dict(kernel_size=K, dilation=D, padding=R * D)
    col = fr.permute(0, 3, 1, 2).float()
    dc = ((F.unfold(col, **kw).view(1, 3, K * K, H * W) - col.reshape(1, 3, 1, H * W)) ** 2).sum(1)
    r = torch.arange(-R, R + 1, device=u.device, dtype=torch.float32) * D
    ds = (r[:, None] ** 2 + r[None, :] ** 2).reshape(1, K * K, 1)
    k = w_a * torch.exp(-(a_s * ds + a_c * dc)) + w_s * torch.exp(-g_s * ds)
    k[:, K * K // 2] = 0.0
    z = u[:, None]
    for _ in range(iters):
        z = u[:, None] + (k * F.unfold(2.0 * torch.sigmoid(z) - 1.0, **kw)).sum(1).view(1, 1, H, W)
    return z[:, 0]


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
    loops, state = [], {}
    forward_at = {}
    for (h, w) in [(480, 854), (1080, 1920)]:
        u, fr = [t.to(device) for t in scene(h, w)]

        def forward(fr=fr):
            with torch.no_grad():
                state["fwd"] = net.forward(augment_frame(fr[0], None, False, None)[0][None])[-1]
        forward_at[(h, w)] = len(loops)
        loops.append(("%4dx%-4d one test forward (augment_frame identity + net.forward)" % (w, h), forward, SLOW_PASSES, None))
        for (R, D) in [(5, 3), (3, 2)]:
            kw = dict(radius=R, dilation=D)
            one, five = refine.CrfRefiner(iters=1, **kw), refine.CrfRefiner(iters=5, **kw)
            out1, out5 = torch.empty_like(u), torch.empty_like(u)
            tag = "%4dx%-4d R %d D %d (%3d neighbours)" % (w, h, R, D, (2 * R + 1) ** 2 - 1)
            loops.append((tag + " kernel, per iteration", lambda one=one, u=u, fr=fr, o=out1: one(u, fr, out=o), PASSES, (h, w)))
            loops.append((tag + " kernel, five iterations", lambda five=five, u=u, fr=fr, o=out5: five(u, fr, out=o), PASSES, (h, w)))

            def plain(u=u, fr=fr, c=five.coeffs, R=R, D=D, tag=tag):
                state[tag] = torch_rule(u, fr, c, 5, R, D)
            loops.append((tag + " torch unfold, five iterations", plain, SLOW_PASSES, (h, w)))
            plain()
            diff = float((state[tag] - five(u, fr)).abs().max())
            state[tag + " diff"] = diff
            assert diff < 1e-3, "the kernel and the torch formulation disagree: %g" % diff
            del state[tag]
    tiny_u, tiny_fr = torch.zeros(1, 1, 1, device=device), torch.zeros(1, 1, 1, 3, device=device, dtype=torch.uint8)
    tiny = refine.CrfRefiner(iters=1)
    tiny_out = torch.empty_like(tiny_u)
    loops.append(("   1x1    R 5 D 3 kernel, per iteration (a launch through the wrapper)", lambda: tiny(tiny_u, tiny_fr, out=tiny_out), PASSES, None))
    for _ in range(WARM):
        for _, fn, _, _ in loops:
            fn()
    times = [[] for _ in loops]
    for _ in range(WINDOWS):
        for i, (_, fn, passes, _) in enumerate(loops):
            times[i].append(window(fn, passes))
    lines = ["command: python tools/time_crf.py   (%s, torch %s, precision %s, GPU_MAX_HW_QUEUES=%s)"
             % (torch.cuda.get_device_name(0), torch.__version__, args.precision, os.environ.get("GPU_MAX_HW_QUEUES", "unset")),
             "batch 1, default weights (4, 1) and thetas (8, 13, 3); us per CALL, median [min .. max] of %d windows of %d calls (%d for the torch"
             % (WINDOWS, PASSES, SLOW_PASSES),
             "formulation and the forward), device events, the loops alternating in one process on one stream; 'x forward' is the ratio of medians to",
             "the forward of the same size in this run.", "colour factor: one hardware exp2 per neighbour:"]
    for i, ((name, _, _, size), t) in enumerate(zip(loops, times)):
        rel = "   x forward %6.3f" % (np.median(t) / np.median(times[forward_at[size]])) if size else ""
        lines.append("  %-72s %s%s" % (name, stats(t), rel))
    for k in sorted(state):
        if k.endswith(" diff"):
            lines.append("  max |torch fp32 - kernel| after five iterations, %s: %.2e" % (k[:-5], state[k]))
    fwd = float(np.median(times[forward_at[(480, 854)]]))
    five = [float(np.median(t)) for (name, _, _, size), t in zip(loops, times) if size == (480, 854) and "R 5 D 3" in name and "kernel, five" in name][0]
    lines.append("aim: the default five iterations at 854x480 cost less than one test forward: %.1f us against %.1f us -- %s by a factor of %.2f"
                 % (five, fwd, "MET" if five < fwd else "MISSED", max(five, fwd) / min(five, fwd)))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
