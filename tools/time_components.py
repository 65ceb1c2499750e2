#!/usr/bin/env python3
"""Time the device-side mask clean-up (results.ComponentTracker: osvos_mask_components + the chained osvos_components_select) next to the route
a user has without it: the logits copied to the host, scipy.ndimage.label + np.bincount + the selection rule in numpy, the mask copied back.

    python tools/time_components.py [--out profiles/components.txt]          (needs the GPU)

Input: the fused logits of `train_online.py --synthetic`'s network after a short fine-tuning on its synthetic 854x480 frame, repeated with
noise so that false-positive blobs appear.  Batch 1 and batch 12; both paths run in the same process on the same tensors, alternating.  The
device path is timed with device events around PASSES back-to-back calls (it never waits for the host); the host path synchronises by nature,
so it is timed with events as well as with the wall clock.  Median [min .. max] of WINDOWS windows, reported per FRAME.  The kept maps of the
two paths must be equal.  bench.py's pipe_sustained figure for the box is taken by the caller and appended to the profile by hand.
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy import ndimage  # noqa: E402

import networks.vgg_osvos as vo  # noqa: E402
from osvos_pytorch_amd import results  # noqa: E402
from osvos_pytorch_amd.train_common import TrainLoop, make_sgd  # noqa: E402

PASSES, WARM, WINDOWS, RADIUS = 10, 2, 5, 8


def fine_tuned_logits(device, h, w, frames, steps):
    from train_online import synthetic_loader
    torch.manual_seed(0)
    s = synthetic_loader(h, w, 0)[0]
    net = vo.OSVOS(pretrained=0).to(device)
    net.set_precision("fp32x3")
    loop = TrainLoop(net, make_sgd(net, "online"), mode="online", n_ave_grad=1)
    img, gt = s["image"].to(device), s["gt"].to(device)
    for _ in range(steps):
        loop.micro_batch(img.detach().requires_grad_(), gt)
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        x = net.forward(img)[-1][0, 0]
    # later frames: the same map under smooth noise of a few blobs' size, so components come and go
    noise = torch.nn.functional.interpolate(torch.randn(frames, 1, h // 16, w // 16, generator=gen), size=(h, w), mode="bilinear")[:, 0]
    scale = float(x.std())
    return (x[None] + 1.5 * scale * noise.to(device)).contiguous(), (gt[0, 0] > 0.5)


def disk(r):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return yy * yy + xx * xx <= r * r


def host_path(x, seed, thr_logit):
    """the chained rule on the host -> kept uint8 CUDA tensor [N,H,W]; seed: host bool [H,W]"""
    a = x.cpu().numpy()
    kept = np.zeros(a.shape, dtype=np.uint8)
    d = disk(RADIUS)
    for n in range(a.shape[0]):
        lab, count = ndimage.label(a[n] > thr_logit, structure=np.ones((3, 3)))
        if seed.any():
            near = ndimage.binary_dilation(seed, structure=d)
            ok = np.zeros(count + 1, dtype=bool)
            ok[np.unique(lab[near])] = True
            ok[0] = False
        else:
            ok = np.ones(count + 1, dtype=bool)
            ok[0] = False
        np.bincount(lab.reshape(-1), minlength=count + 1)          # the areas a min_area rule would read
        kept[n] = ok[lab]
        seed = kept[n] != 0
    return torch.from_numpy(kept).to(x.device), seed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    device = torch.device("cuda:0")
    h, w = 480, 854
    logits, first = fine_tuned_logits(device, h, w, 12, args.steps)
    first_host = first.cpu().numpy()
    lines = ["command: python tools/time_components.py   (%s, torch %s)" % (torch.cuda.get_device_name(0), torch.__version__),
             "%dx%d fused logits of the synthetic frame after %d fine-tuning steps plus smooth noise, 8-connectivity, seed radius %d, chained;"
             % (w, h, args.steps, RADIUS),
             "us per FRAME, median [min .. max] of %d windows of %d calls, the two paths alternating in one process, one stream." % (WINDOWS, PASSES)]
    for batch in (1, 12):
        x = logits[:batch].contiguous()
        state = {}

        def dev():
            tr = results.ComponentTracker(first, RADIUS)
            state["dev"] = tr(x)

        def host():
            state["host"], _ = host_path(x, first_host, 0.0)

        def window(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            for _ in range(PASSES):
                fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3 / (PASSES * batch), (time.perf_counter() - t0) * 1e6 / (PASSES * batch)

        for _ in range(WARM):
            dev()
            host()
        td, th = [], []
        for _ in range(WINDOWS):
            td.append(window(dev))
            th.append(window(host))
        kept_dev = (state["dev"] > 0.0).to(torch.uint8)             # dropped pixels hold -inf, background sits below the threshold
        same = bool(torch.equal(kept_dev, state["host"]))
        _, _, stats = results.components(x)
        st = stats.cpu().numpy()
        de, he, hw = [t[0] for t in td], [t[0] for t in th], [t[1] for t in th]
        lines += ["batch %2d: components per frame %s, kept pixels %d of %d foreground" % (batch, st[:, 0].tolist(), int(kept_dev.sum()), int(st[:, 1].sum())),
                  "  ComponentTracker (osvos_mask_components + chained osvos_components_select), device events %9.2f [%9.2f .. %9.2f]"
                  % (np.median(de), min(de), max(de)),
                  "  .cpu() + scipy.ndimage.label + bincount + rule in numpy + mask copied back, device events %9.2f [%9.2f .. %9.2f]"
                  % (np.median(he), min(he), max(he)),
                  "  the same, wall clock                                                                      %9.2f [%9.2f .. %9.2f]"
                  % (np.median(hw), min(hw), max(hw)),
                  "  ratio host / device %.1f;  kept maps equal: %s" % (np.median(he) / np.median(de), same)]
        assert same, "the two paths disagree"
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
