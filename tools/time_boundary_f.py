#!/usr/bin/env python3
"""Time the J&F count call (osvos_mask_jf_counts, csrc/boundary.hip) next to the J count call (osvos_mask_iou_counts, csrc/loss.hip -- it
reads the same two float tensors once and is the bandwidth floor of this job), and the test loop of train_online.py with the per-frame
`jaccard` read-back against the device-resident SequenceEvaluator.

    python tools/time_boundary_f.py [--out profiles/boundary_f.txt]          (needs the GPU)

Inputs: the fused logits of a real forward -- the synthetic ellipse frame of train_online.py after 10 fine-tune epochs at 854x480 -- and, because
ten epochs from a random start may leave a mask with little or no boundary, a second set with work in it: the same ellipse as ground truth
against itself moved 9 px, under noisy logits.  Times are device events around 200 back-to-back calls after 20 warm-up calls, the two calls
alternating, median of 7 such windows.
"""
import argparse
import ctypes as C
import os
import sys
import tempfile
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import networks.vgg_osvos as vo  # noqa: E402
from osvos_pytorch_amd import _lib, results  # noqa: E402
from osvos_pytorch_amd.train_common import TrainLoop, make_sgd  # noqa: E402
from train_online import synthetic_loader  # noqa: E402

CALLS, WARM, WINDOWS = 200, 20, 7


def window_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS


def time_pair(x, g, radius):
    l = _lib.lib()
    n, h, w = x.shape[0], x.shape[-2], x.shape[-1]
    ws = torch.empty(l.osvos_boundary_ws_bytes(n, h, w) // 8, device=x.device, dtype=torch.int64)
    c6 = torch.empty((n, 6), device=x.device, dtype=torch.int64)
    c2 = torch.empty((n, 2), device=x.device, dtype=torch.int64)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xp, gp = C.c_void_p(x.data_ptr()), C.c_void_p(g.data_ptr())

    def jf():
        _lib.check(l.osvos_mask_jf_counts(xp, gp, C.c_void_p(ws.data_ptr()), C.c_void_p(c6.data_ptr()), n, h, w, 0.0, radius, 0, st))

    def iou():
        _lib.check(l.osvos_mask_iou_counts(xp, gp, C.c_void_p(c2.data_ptr()), h * w, n, 0.0, st))
    for _ in range(WARM):
        jf()
        iou()
    torch.cuda.synchronize()
    tj, ti = [], []
    for _ in range(WINDOWS):
        tj.append(window_us(jf))
        ti.append(window_us(iou))
    torch.cuda.synchronize()
    assert np.array_equal(c6.cpu().numpy()[:, :2], c2.cpu().numpy())
    return tj, ti, c6.cpu().numpy()


def fine_tuned_net(device, epochs=10):
    net = vo.OSVOS(pretrained=0)
    net.to(device)
    net.set_precision("fp32x3")
    loop = TrainLoop(net, make_sgd(net, "online"), mode="online", n_ave_grad=5)
    s = synthetic_loader(480, 854, 0)[0]
    for _ in range(epochs):
        loop.micro_batch(s["image"].to(device).requires_grad_(), s["gt"].to(device))
    torch.cuda.synchronize()
    return net


def forward_inputs(net, device, n, h, w):
    frames = [synthetic_loader(h, w, i)[0] for i in range(n)]
    with torch.no_grad():
        x = torch.cat([net.forward(f["image"].to(device))[-1] for f in frames]).contiguous()
    return x, torch.cat([f["gt"] for f in frames]).to(device).contiguous()


def shifted_inputs(device, n, h, w):
    gen = torch.Generator().manual_seed(3)
    gt = synthetic_loader(h, w, 0)[0]["gt"]
    x = torch.cat([(torch.roll(gt, 9 + i, dims=3) * 2 - 1) * (0.05 + 4 * torch.rand(1, 1, h, w, generator=gen)) for i in range(n)])
    return x.to(device).contiguous(), gt.repeat(n, 1, 1, 1).to(device).contiguous()


def test_loop(net, device, frames, mode, save_dir):
    """the test loop of train_online.py over `frames` copies of the synthetic frame: forward, result PNG (None: skipped), evaluation"""
    s = synthetic_loader(480, 854, 0)[0]
    img, gt = s["image"].to(device), s["gt"].to(device)
    ev, js = results.SequenceEvaluator(), []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        for i in range(frames):
            out = net.forward(img)
            if save_dir:
                results.save_masks(out[-1], [os.path.join(save_dir, "%05d.png" % i)])
            if mode == "jaccard":
                js.extend(results.jaccard(out[-1], gt))
            else:
                ev.add(out[-1], gt)
    if mode != "jaccard":
        js = ev.per_frame()[0]
    torch.cuda.synchronize()
    return frames / (time.perf_counter() - t0), js


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--loop-frames", type=int, default=200)
    ap.add_argument("--kernels-only", default="", metavar="N,H,W",
                    help="only the count calls at one size on the moved-ellipse input, no network: the run to put under rocprofv3 --kernel-trace --stats")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    device = torch.device("cuda:0")
    if args.kernels_only:
        n, h, w = [int(v) for v in args.kernels_only.split(",")]
        x, g = shifted_inputs(device, n, h, w)
        tj, ti, c = time_pair(x, g, results.boundary_radius(h, w))
        print("%dx%d N %d: J&F %.1f us, J %.1f us per call (under the profiler if one is attached)" % (w, h, n, np.median(tj), np.median(ti)))
        return
    lines = ["command: python tools/time_boundary_f.py   (%s, torch %s)" % (torch.cuda.get_device_name(0), torch.__version__),
             "osvos_mask_jf_counts (memset + jf_pack_kernel + jf_match_kernel) against osvos_mask_iou_counts (memset + mask_iou_kernel; loss.hip is",
             "untouched by this change, so this IS the parent commit's kernel); us per call, device events around %d calls, median [min .. max] of %d windows"
             % (CALLS, WINDOWS), ""]
    net = fine_tuned_net(device)
    for label, make in (("fused logits of a real forward (synthetic ellipse, 10 fine-tune epochs)", lambda n, h, w: forward_inputs(net, device, n, h, w)),
                        ("ellipse moved 9+ px under noisy logits", lambda n, h, w: shifted_inputs(device, n, h, w))):
        lines.append(label)
        for (n, h, w) in ((1, 480, 854), (12, 480, 854), (4, 1080, 1920)):
            x, g = make(n, h, w)
            r = results.boundary_radius(h, w)
            tj, ti, c = time_pair(x, g, r)
            lines.append("  %4dx%-4d N %2d r %2d   J&F %7.1f [%6.1f .. %6.1f]   J %7.1f [%6.1f .. %6.1f]   ratio %.2f   frame 0: n_fb %d n_gb %d matched %d / %d"
                         % (w, h, n, r, np.median(tj), min(tj), max(tj), np.median(ti), min(ti), max(ti), np.median(tj) / np.median(ti),
                            c[0, 2], c[0, 3], c[0, 4], c[0, 5]))
            del x, g
        lines.append("")
    lines.append("test loop of train_online.py at 854x480 fp32x3, %d frames, frames/s (host clock, ends in a synchronise), alternating runs:" % args.loop_frames)
    with tempfile.TemporaryDirectory() as tmp:
        test_loop(net, device, 20, "jaccard", tmp)
        test_loop(net, device, 20, "evaluator", tmp)
        for save in (tmp, None):
            rates = {"jaccard": [], "evaluator": []}
            for _ in range(3):
                for mode in ("jaccard", "evaluator"):
                    fps, js = test_loop(net, device, args.loop_frames, mode, save)
                    rates[mode].append(fps)
            lines.append("  %-28s jaccard per frame (parent loop) %s   SequenceEvaluator %s"
                         % ("with result PNGs:" if save else "evaluation only (no PNGs):", " ".join("%.1f" % v for v in rates["jaccard"]),
                            " ".join("%.1f" % v for v in rates["evaluator"])))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
