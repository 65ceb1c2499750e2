#!/usr/bin/env python3
"""Time the superpixel snapping (osvos_pytorch_amd.superpixels -> osvos_superpixels_slic / osvos_superpixels_pool, csrc/superpixels.hip)
next to one test forward of the network, the step it runs behind, and next to a torch formulation of the same rule.

    python tools/time_superpixels.py [--out profiles/superpixels_timing.txt]          (needs the GPU)

A seeded 854x480 frame (flat regions under +-12 colour noise) and noise logits, N = 1; the default parameters (cell 8, compactness 10,
iters 5).  The torch formulation states the same integer rule with tensor operations -- the nine candidates gathered from the centre table
and compared in ascending k with a strict <, the sums by index_add_ on int64 -- with everything that depends on the geometry alone made
once outside the timed loop; its labels and pooled logits are checked equal to the kernels' before anything is timed.  All loops run in one
process on one stream, alternating window by window; device events around PASSES back-to-back calls (nothing waits for the host inside a
window).  Median [min .. max] of WINDOWS windows.  The per-kernel times come from one torch.profiler trace of ten snapper calls.  The forward
runs an untrained network (a forward's time does not depend on the weights) at train_online.py's default test precision.  There is no bar:
the numbers are recorded, and the only claims made from them are the ratios to the forward and to the torch formulation of the same run.
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
from osvos_pytorch_amd import superpixels  # noqa: E402
from osvos_pytorch_amd.augment import augment_frame  # noqa: E402

PASSES, WARM, WINDOWS = 20, 3, 7
SLOW_PASSES = 5          # the forward and the torch formulation: milliseconds per call
H, W = 480, 854
KERNELS = ("assign_kernel<true>", "assign_kernel<false>", "update_kernel", "pool_accumulate", "pool_apply")


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
    """uint8 [1,H,W,3]: a few flat regions with curved borders under +-12 colour noise, and float32 [1,H,W] noise logits"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    region = ((xx - 300) ** 2 + (yy - 200) ** 2 < 150 ** 2).astype(int) + (np.sin(xx / 40.0) * 60 + 300 < yy).astype(int)
    pal = np.array([(120, 130, 60), (40, 90, 200), (200, 60, 90)])
    frame = np.clip(pal[region] + rng.integers(-12, 13, size=(H, W, 3)), 0, 255).astype(np.uint8)
    logits = (rng.standard_normal((1, H, W)) * 4).astype(np.float32)
    return torch.from_numpy(frame[None]), torch.from_numpy(logits)


class TorchSlic(object):
    """the rule of include/osvos_hip.h in torch tensor operations, for one frame; the geometry is prepared once"""

    def __init__(self, frame, cell, compactness):
        dev = frame.device
        h, w = int(frame.shape[0]), int(frame.shape[1])
        self.gh, self.gw = superpixels.grid_shape(h, w, cell)
        self.k = self.gh * self.gw
        self.s2, self.m2 = cell * cell, compactness * compactness
        yy, xx = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
        self.xx, self.yy = xx, yy
        self.px = frame.long()
        self.comp = torch.cat([xx[..., None], yy[..., None], self.px, torch.ones_like(xx)[..., None]], -1).reshape(-1, 6)
        gy, gx = yy // cell, xx // cell
        self.home = gy * self.gw + gx
        self.cand = []
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                cy, cx = gy + oy, gx + ox
                ok = (cy >= 0) & (cy < self.gh) & (cx >= 0) & (cx < self.gw)
                self.cand.append((cy.clamp(0, self.gh - 1) * self.gw + cx.clamp(0, self.gw - 1), ok))

    def update(self, labels, prev):
        sums = torch.zeros((self.k, 6), device=labels.device, dtype=torch.int64).index_add_(0, labels.reshape(-1), self.comp)
        count = sums[:, 5:6]
        c = (2 * sums[:, :5] + count) // (2 * count.clamp(min=1))
        if prev is not None:
            c = torch.where(count > 0, c, prev[:, :5])
        return torch.cat([c, count], 1)

    def assign(self, centres):
        best = torch.full_like(self.home, 2 ** 62)
        lab = torch.zeros_like(self.home)
        for k, ok in self.cand:
            c = centres[k]
            d = self.s2 * ((self.px - c[..., 2:5]) ** 2).sum(-1) + self.m2 * ((self.xx - c[..., 0]) ** 2 + (self.yy - c[..., 1]) ** 2)
            better = ok & (d < best)
            best = torch.where(better, d, best)
            lab = torch.where(better, k, lab)
        return lab

    def __call__(self, iters):
        labels = self.home
        centres = self.update(labels, None)
        for _ in range(iters):
            labels = self.assign(centres)
            centres = self.update(labels, centres)
        return labels


def torch_pool(logits, labels, k):
    """logits float32 [H,W], labels int64 [H,W] in [0, k) -> float32 [H,W], the pooling rule in torch tensor operations"""
    x = torch.where(torch.isnan(logits), torch.full_like(logits, -16384.0), logits.clamp(-16384.0, 16384.0))
    q = torch.round(x * 65536.0).long().reshape(-1)
    lab = labels.reshape(-1)
    sums = torch.zeros(k, device=logits.device, dtype=torch.int64).index_add_(0, lab, q)
    count = torch.zeros(k, device=logits.device, dtype=torch.int64).index_add_(0, lab, torch.ones_like(q))
    mean = (2 * sums + count) // (2 * count.clamp(min=1))
    return (mean.float() * (1.0 / 65536.0))[lab].reshape(logits.shape)


def kernel_of(key):
    """the entry of KERNELS a trace event's name stands for (demangled or mangled), or None"""
    for base in ("assign_kernel", "update_kernel", "pool_accumulate", "pool_apply"):
        if base in key:
            if base == "assign_kernel":
                return base + ("<true>" if ("<true>" in key or "ILb1E" in key) else "<false>")
            return base
    return None


def kernel_times(fn, calls=10):
    """{kernel name fragment: (launches per call, us per launch)} from one torch.profiler trace of `calls` calls, or a text saying why not"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        seen = {}
        for e in prof.key_averages():
            total = getattr(e, "self_device_time_total", None)
            if total is None:
                total = getattr(e, "self_cuda_time_total", 0)
            name = kernel_of(e.key)
            if name and total > 0:
                count, us = seen.get(name, (0, 0.0))
                seen[name] = (count + e.count, us + total)
        out = {name: (count / float(calls), us / count) for name, (count, us) in seen.items()}
        return out if out else "the profiler trace held none of the kernels"
    except Exception as e:          # the trace is a convenience of this tool: say so and go on with the event times
        return "torch.profiler failed: %s" % e


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
    frames, logits = [t.to(device) for t in scene()]
    kw = dict(cell=8, compactness=10, iters=5)
    gh, gw = superpixels.grid_shape(H, W, kw["cell"])
    k = gh * gw
    state = {}

    def forward():
        with torch.no_grad():
            state["fwd"] = net.forward(augment_frame(frames[0], None, False, None)[0][None])[-1]

    ws = superpixels.slic_workspace(1, H, W, kw["cell"], device)
    pws = superpixels.pool_workspace(1, k, device)
    labels = superpixels.slic(frames, ws=ws, **kw)
    pooled = superpixels.pool(logits, labels, k, ws=pws)
    ts = TorchSlic(frames[0], kw["cell"], kw["compactness"])
    tlabels = ts(kw["iters"])
    assert torch.equal(tlabels, labels[0].long()), "the torch formulation and the kernels disagree on the labels"
    assert torch.equal(torch_pool(logits[0], tlabels, k), pooled[0]), "the torch formulation and the kernels disagree on the pooled logits"
    snapper = superpixels.SuperpixelSnapper(**kw)
    assert torch.equal(snapper(logits, frames), pooled)

    loops = [("854x480 one test forward (augment_frame identity + net.forward)", forward, SLOW_PASSES),
             ("854x480 cell 8 compactness 10 iters 5 (%d superpixels) slic" % k, lambda: superpixels.slic(frames, ws=ws, **kw), PASSES),
             ("854x480 the same with iters 0 (memset, labels_0, one update)", lambda: superpixels.slic(frames, 8, 10, 0, ws=ws), PASSES),
             ("854x480 pool over those labels", lambda: superpixels.pool(logits, labels, k, ws=pws), PASSES),
             ("854x480 SuperpixelSnapper (slic + pool)", lambda: snapper(logits, frames), PASSES),
             ("854x480 torch formulation of slic (nine-candidate gather + index_add_)", lambda: ts(kw["iters"]), SLOW_PASSES),
             ("854x480 torch formulation of pool (index_add_ + gather)", lambda: torch_pool(logits[0], tlabels, k), PASSES)]
    for _ in range(WARM):
        for _, fn, _ in loops:
            fn()
    times = [[] for _ in loops]
    for _ in range(WINDOWS):
        for i, (_, fn, passes) in enumerate(loops):
            times[i].append(window(fn, passes))
    lines = ["command: python tools/time_superpixels.py   (%s, torch %s, precision %s, GPU_MAX_HW_QUEUES=%s)"
             % (torch.cuda.get_device_name(0), torch.__version__, args.precision, os.environ.get("GPU_MAX_HW_QUEUES", "unset")),
             "batch 1, flat regions under +-12 colour noise, noise logits; us per CALL through the Python wrapper (every launch of the call, output",
             "allocation included), median [min .. max] of %d windows of %d calls (%d for the forward and the torch slic), device events, the loops"
             % (WINDOWS, PASSES, SLOW_PASSES),
             "alternating in one process on one stream; 'x forward' is the ratio of medians to the forward of this run.  The torch formulation",
             "gave the kernels' labels and pooled logits bit for bit before the timing.  No bar is set: recorded, not gated."]
    med = [float(np.median(t)) for t in times]
    for (name, _, _), t in zip(loops, times):
        lines.append("  %-78s %s   x forward %6.3f" % (name, stats(t), np.median(t) / med[0]))
    lines.append("  per assign + update step, from iters 5 against iters 0: %.1f us" % ((med[1] - med[2]) / 5.0))
    lines.append("  torch formulation / kernels: slic %.1fx, pool %.1fx" % (med[5] / med[1], med[6] / med[3]))
    kt = kernel_times(lambda: snapper(logits, frames))
    if isinstance(kt, str):
        lines.append("per kernel: not measured (%s)" % kt)
    else:
        lines.append("per kernel, device time from one torch.profiler trace of ten SuperpixelSnapper calls (launches per call, us per launch):")
        for frag in KERNELS:
            if frag in kt:
                lines.append("  %-24s %4.1f x %8.1f us" % ((frag,) + kt[frag]))
            else:
                lines.append("  %-24s not in the trace" % frag)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
