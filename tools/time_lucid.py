#!/usr/bin/env python3
"""Time the lucid first-frame synthesis (osvos_pytorch_amd.lucid -> osvos_lucid_compose / osvos_lucid_inpaint, csrc/lucid.hip) next to the
call it stands in for -- the osvos_augment_frame warp -- next to a torch formulation of the same composition, and next to the training step
it feeds.

    python tools/time_lucid.py [--out profiles/lucid_timing.txt]          (needs the GPU)

A seeded 854x480 frame (a textured ellipse on a gradient under +-12 colour noise) and LucidDream with the default parameters; the sixteen
parameter sets of the timed calls are drawn once with random.seed(0).  The torch formulation is grid_sample (bilinear, align_corners) per
layer on float tensors plus tone and blend: the same composition in floats, not the same bits -- its image is checked to lie within four grey
levels of the kernel's on at least 99 % of the words before anything is timed (its coordinates are not the 5-bit fixed-point ones).  All
loops run in one process on one stream, alternating window by window; device events around PASSES back-to-back calls (nothing waits for the
host inside a window).  Median [min .. max] of WINDOWS windows.  The training step is TrainLoop.micro_batch with one optimizer step each on
an untrained network (a step's time does not depend on the weights).  There is no bar: the numbers are recorded, and the only claims
made from them are the ratios of the same run.
"""
import argparse
import os
import random
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import networks.vgg_osvos as vo  # noqa: E402
from osvos_pytorch_amd import lucid  # noqa: E402
from osvos_pytorch_amd.augment import MEANVAL, augment_frame  # noqa: E402
from osvos_pytorch_amd.train_common import TrainLoop, make_sgd  # noqa: E402

PASSES, WARM, WINDOWS = 20, 3, 7
SLOW_PASSES = 5          # the training step: milliseconds per call
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
    """uint8 [H,W,3] and uint8 [H,W]: a textured ellipse on a gradient under +-12 colour noise, and its mask"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    inside = ((yy - 0.5 * H) / (0.25 * H)) ** 2 + ((xx - 0.45 * W) / (0.2 * W)) ** 2 <= 1
    back = np.stack([60 + xx // 6, 90 + yy // 5, 40 + (xx + yy) // 12], -1)
    tex = np.where((((yy // 7) + (xx // 7)) % 2 == 0)[..., None], (40, 60, 220), (70, 30, 180))
    frame = np.clip(np.where(inside[..., None], tex, back) + rng.integers(-12, 13, size=(H, W, 3)), 0, 255).astype(np.uint8)
    return torch.from_numpy(frame), torch.from_numpy(inside.astype(np.uint8) * 255)


class TorchCompose(object):
    """the composition in torch tensor operations on floats, for one sample; what depends on the frame alone is prepared once"""

    def __init__(self, frame, mask, bg):
        self.h, self.w = int(mask.shape[0]), int(mask.shape[1])
        self.fg = torch.cat([frame.permute(2, 0, 1).float(), (mask != 0).float()[None]])[None]      # [1,4,H,W]: colours and alpha
        self.bg = bg.permute(2, 0, 1).float()[None]
        self.mean = torch.tensor(MEANVAL, device=frame.device).view(1, 3, 1, 1)
        yy, xx = torch.meshgrid(torch.arange(self.h, device=frame.device, dtype=torch.float32),
                                torch.arange(self.w, device=frame.device, dtype=torch.float32), indexing="ij")
        self.xy1 = torch.stack([xx, yy, torch.ones_like(xx)], -1)                                      # [H,W,3]
        self.scale = torch.tensor([2.0 / max(self.w - 1, 1), 2.0 / max(self.h - 1, 1)], device=frame.device)

    def grid(self, m):
        src = self.xy1 @ torch.tensor([[m[0], m[3]], [m[1], m[4]], [m[2], m[5]]], device=self.xy1.device, dtype=torch.float32)
        return (src * self.scale - 1.0)[None]

    def __call__(self, matrices, tones):
        fg = F.grid_sample(self.fg, self.grid(matrices[0]), mode="bilinear", padding_mode="zeros", align_corners=True)
        col = F.grid_sample(self.fg[:, :3], self.grid(matrices[0]), mode="bilinear", padding_mode="border", align_corners=True)
        bg = F.grid_sample(self.bg, self.grid(matrices[1]), mode="bilinear", padding_mode="border", align_corners=True)
        t = torch.tensor(tones, device=fg.device, dtype=torch.float32)
        col = (col * (t[0, :3] / 256.0).view(1, 3, 1, 1) + t[0, 3:].view(1, 3, 1, 1)).clamp(0, 255)
        bg = (bg * (t[1, :3] / 256.0).view(1, 3, 1, 1) + t[1, 3:].view(1, 3, 1, 1)).clamp(0, 255)
        a = fg[:, 3:4]
        return a * col + (1 - a) * bg - self.mean, (a >= 0.5).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--precision", default="fp32x3")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    random.seed(0)
    net = vo.OSVOS(pretrained=0).to(device)
    net.set_precision(args.precision)
    loop = TrainLoop(net, make_sgd(net, "online"), mode="online", n_ave_grad=1)
    frame, mask = [t.to(device) for t in scene()]
    dream = lucid.LucidDream(frame, mask)
    draws = [dream.draw() for _ in range(16)]
    M, T = [d[0] for d in draws], [d[1] for d in draws]
    image, gt = lucid.compose(frame, mask, dream.bg, M[:1], T[:1])
    tc = TorchCompose(frame, mask, dream.bg)
    t_image, t_gt = tc(M[0], T[0])
    near = float(((t_image - image).abs() <= 4.0).float().mean())
    same_gt = float((t_gt == gt).float().mean())
    assert near >= 0.99 and same_gt >= 0.999, "the torch formulation and the kernel disagree: %.5f of the image within 4, %.5f of the labels" % (near, same_gt)
    hole_px = int(dream.hole.sum())
    ws = torch.empty((lucid.lib().osvos_lucid_inpaint_ws_bytes(H, W, dream.passes) + 3) // 4, device=device, dtype=torch.int32)
    sample = {"image": image.clone(), "gt": gt.clone()}

    def step():
        loop.micro_batch(sample["image"].detach().requires_grad_(), sample["gt"])

    def raw(n, matrices, tones):
        """osvos_lucid_compose alone: arguments and outputs prepared once, so that a window times the launches and not the wrapper"""
        import ctypes as C
        m, t = np.ascontiguousarray(np.asarray(matrices[:n], np.float64)), np.ascontiguousarray(np.asarray(tones[:n], np.int32))
        out_img, out_gt = torch.empty((n, 3, H, W), device=device), torch.empty((n, 1, H, W), device=device)
        mean, vp, fn = (C.c_float * 3)(*MEANVAL), C.c_void_p, lucid.lib().osvos_lucid_compose
        a = (vp(frame.data_ptr()), vp(mask.data_ptr()), vp(dream.bg.data_ptr()), vp(m.ctypes.data), vp(t.ctypes.data), mean, vp(out_img.data_ptr()),
             vp(out_gt.data_ptr()), n, H, W, vp(torch.cuda.current_stream().cuda_stream))
        keep = (m, t, out_img, out_gt, mean)

        def call():
            assert fn(*a) == 0, keep is None
        return call
    ident = [[lucid.IDENTITY, lucid.IDENTITY]] * 16

    loops = [("854x480 fp32x3 training step (TrainLoop.micro_batch, one optimizer step)", step, SLOW_PASSES),
             ("854x480 augment_frame, flip + rotate 17 deg + scale 1.1 (the existing sample)", lambda: augment_frame(frame, mask, True, 17.0, 1.1), PASSES),
             ("854x480 lucid.compose, N = 1", lambda: lucid.compose(frame, mask, dream.bg, M[:1], T[:1]), PASSES),
             ("854x480 lucid.compose, N = 16 in one launch", lambda: lucid.compose(frame, mask, dream.bg, M, T), PASSES),
             ("854x480 torch formulation, N = 1 (3 grid_sample + tone + blend)", lambda: tc(M[0], T[0]), PASSES),
             ("854x480 lucid.inpaint radius %d passes %d, hole of %d pixels" % (dream.radius, dream.passes, hole_px),
              lambda: lucid.inpaint(frame, dream.hole, dream.radius, dream.passes, ws=ws), PASSES),
             ("854x480 lucid.inpaint passes 0 (column pass + row pass)", lambda: lucid.inpaint(frame, dream.hole, dream.radius, 0, ws=ws), PASSES),
             ("854x480 osvos_lucid_compose alone, N = 1, drawn parameters", raw(1, M, T), PASSES),
             ("854x480 osvos_lucid_compose alone, N = 16, drawn parameters", raw(16, M, T), PASSES),
             ("854x480 osvos_lucid_compose alone, N = 16, identity matrices (every tap read coalesced)", raw(16, ident, T), PASSES)]
    for _ in range(WARM):
        for _, fn, _ in loops:
            fn()
    times = [[] for _ in loops]
    for _ in range(WINDOWS):
        for i, (_, fn, passes) in enumerate(loops):
            times[i].append(window(fn, passes))
    lines = ["command: python tools/time_lucid.py   (%s, torch %s, precision %s, GPU_MAX_HW_QUEUES=%s)"
             % (torch.cuda.get_device_name(0), torch.__version__, args.precision, os.environ.get("GPU_MAX_HW_QUEUES", "unset")),
             "a textured ellipse on a gradient under +-12 colour noise, LucidDream defaults, 16 parameter sets drawn with random.seed(0); us per",
             "CALL through the Python wrapper (every launch of the call, output allocation and parameter checks included; the rows 'alone' call the",
             "library with arguments and outputs prepared once), median [min .. max] of",
             "%d windows of %d calls (%d for the training step), device events, the loops alternating in one process on one stream; 'x step' is"
             % (WINDOWS, PASSES, SLOW_PASSES),
             "the ratio of medians to the training step of this run.  The torch formulation is the same composition in floats (%.3f %% of its image"
             % (100 * near),
             "words within four grey levels of the kernel's, %.3f %% of its labels equal); it is not bit-exact.  No bar is set: recorded, not gated."
             % (100 * same_gt)]
    med = [float(np.median(t)) for t in times]
    for (name, _, _), t in zip(loops, times):
        lines.append("  %-82s %s   x step %7.4f" % (name, stats(t), np.median(t) / med[0]))
    lines.append("  compose per sample at N = 16: %.1f us; compose N = 1 / augment_frame: %.2fx; torch formulation / compose N = 1: %.2fx"
                 % (med[3] / 16.0, med[2] / med[1], med[4] / med[2]))
    lines.append("  the kernel alone at N = 16: %.1f us per sample with the drawn rotations, %.1f us with identity matrices (the same stores, no gather): "
                 "gather cost %.1f %%" % (med[8] / 16.0, med[9] / 16.0, 100.0 * (med[8] - med[9]) / med[9]))
    lines.append("  per smoothing pass, from passes %d against passes 0: %.1f us" % (dream.passes, (med[5] - med[6]) / max(dream.passes, 1)))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
