#!/usr/bin/env python3
"""Time appearance matching (osvos_pytorch_amd.match -> osvos_match_quantize / osvos_match_nearest, csrc/match.hip) next to one test forward of
the network, the step it rides on, and report how much the int8 quantisation moves a cosine.

    python tools/time_match.py [--out profiles/match_timing.txt]          (needs the GPU)

A seeded 854x480 frame, N = 1.  The features are the network's own: conv4_3 (layer 9: 60 x 107 = 6420 pixels of 512 channels) and conv3_3
(layer 6: 120 x 214 = 25680 pixels of 256 channels) of an untrained network (a kernel's time does not depend on the values), searched
against the same frame's features under a half-and-half labelling.  All loops run in one process on one stream, alternating window by
window; device events around PASSES back-to-back calls (nothing waits for the host inside a window).  Median [min .. max] of WINDOWS windows.
The int8 op rate counts 2 Pq Pr C operations per nearest call.  The forward runs at train_online.py's default test precision.  There is no
bar: the numbers are recorded, and the only claims made from them are the ratios to the forward of the same run.

The distortion figure: on conv4_3 of the trained-like fixture of the test suite (tests/trained_fixture.py, trained on the device in this run;
if that fails, on the untrained network, and the output says so), for SAMPLE random pixel pairs, |cos_q - cos_f64| with cos_q the cosine of
the int8 vectors as the kernels form it and cos_f64 the float64 cosine of the fp32 features.  Reported, not gated.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tests"))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import networks.vgg_osvos as vo  # noqa: E402
from osvos_pytorch_amd import match  # noqa: E402
from osvos_pytorch_amd.augment import augment_frame  # noqa: E402

PASSES, WARM, WINDOWS = 20, 3, 7
SLOW_PASSES = 5          # the forward, the matcher and the layer-6 search: a millisecond or more per call
H, W = 480, 854
SAMPLE = 20000


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


def distortion(net, x, layer, what):
    """one line: the largest and mean |cos_q - cos_f64| over SAMPLE random pairs of the pixels of trunk tensor `layer` of x"""
    feat = net.forward_features(x, layer)[1]
    c = int(feat.shape[-1])
    q, rinv = match.quantize(feat)
    f = feat.float().reshape(-1, c).cpu().numpy().astype(np.float64)
    q, rinv = q.reshape(-1, c).cpu().numpy().astype(np.float64), rinv.reshape(-1).cpu().numpy().astype(np.float64)
    live = np.flatnonzero((np.abs(f).max(axis=1) > 0) & (rinv > 0))
    rng = np.random.default_rng(1)
    a, b = rng.choice(live, SAMPLE), rng.choice(live, SAMPLE)
    norm = np.sqrt((f * f).sum(axis=1))
    cos_f = (f[a] * f[b]).sum(axis=1) / (norm[a] * norm[b])
    cos_q = (q[a] * q[b]).sum(axis=1) * rinv[a] * rinv[b]
    d = np.abs(cos_q - cos_f)
    return ("  %s, layer %d (%d live pixels of %d, C %d), %d random pairs: |cos_q - cos_f64| largest %.3e, mean %.3e (cosines %.3f .. %.3f)"
            % (what, layer, live.size, f.shape[0], c, SAMPLE, d.max(), d.mean(), cos_f.min(), cos_f.max()))


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
    x = augment_frame(frame, None, False, None)[0][None]
    state = {}

    def forward():
        with torch.no_grad():
            state["fwd"] = net.forward(augment_frame(frame, None, False, None)[0][None])[-1]

    mask = torch.zeros((1, H, W), device=device, dtype=torch.uint8)
    mask[:, :, :W // 2] = 1
    loops = [("854x480 one test forward (augment_frame identity + net.forward)", forward, SLOW_PASSES, 0)]
    keep = []
    for layer in (9, 6):
        feat = net.forward_features(x, layer)[1].clone()
        n, h, w, c = (int(v) for v in feat.shape)
        p = h * w
        q, rinv = match.quantize(feat)
        q, rinv = q.view(1, p, c), rinv.view(1, p)
        label = match.cell_labels(mask, match.stride_of(layer)).view(1, p)
        ws = match.nearest_workspace(1, p, p, c, device)
        slices = ws.numel() // (2 * p * 8)
        keep.append((feat, q, rinv, label, ws))
        loops.append(("layer %d quantize (%d x %d = %d pixels, C %d, %s)" % (layer, h, w, p, c, str(feat.dtype).replace("torch.", "")),
                      lambda feat=feat: match.quantize(feat), PASSES, 0))
        loops.append(("layer %d nearest (%d x %d x %d, %d slices of the reference rows)" % (layer, p, p, c, slices),
                      lambda q=q, rinv=rinv, label=label, ws=ws: match.nearest(q, rinv, q, rinv, label, ws=ws), PASSES if layer == 9 else SLOW_PASSES,
                      2.0 * p * p * c))
    matcher = match.AppearanceMatcher(net, 9, 4.0).set_reference(x, mask)
    loops.append(("854x480 AppearanceMatcher at layer 9 (augment_frame + forward_features + quantize + nearest + fuse)",
                  lambda: matcher(augment_frame(frame, None, False, None)[0][None]), SLOW_PASSES, 0))
    for _ in range(WARM):
        for _, fn, _, _ in loops:
            fn()
    times = [[] for _ in loops]
    for _ in range(WINDOWS):
        for i, (_, fn, passes, _) in enumerate(loops):
            times[i].append(window(fn, passes))
    lines = ["command: python tools/time_match.py   (%s, torch %s, precision %s, GPU_MAX_HW_QUEUES=%s)"
             % (torch.cuda.get_device_name(0), torch.__version__, args.precision, os.environ.get("GPU_MAX_HW_QUEUES", "unset")),
             "batch 1, the features of an untrained network on a seeded frame, searched against themselves under a half-and-half labelling; us per CALL",
             "through the Python wrapper (every launch of the call, output allocation included), median [min .. max] of %d windows of %d calls (%d for"
             % (WINDOWS, PASSES, SLOW_PASSES),
             "the forward, the matcher and the layer-6 search), device events, the loops alternating in one process on one stream; 'x forward' is the",
             "ratio of medians to the forward of this run; the int8 rate counts 2 Pq Pr C operations per call.  No bar is set: recorded, not gated."]
    med = [float(np.median(t)) for t in times]
    for (name, _, _, ops), t in zip(loops, times):
        rate = "   %7.1f int8 Top/s" % (ops / (np.median(t) * 1e-6) / 1e12) if ops else ""
        lines.append("  %-100s %s   x forward %6.3f%s" % (name, stats(t), np.median(t) / med[0], rate))
    lines.append("  matcher minus forward: %.1f us (%.3f of the forward)" % (med[-1] - med[0], (med[-1] - med[0]) / med[0]))
    lines.append("int8 quantisation against the float64 cosine (reported, not gated):")
    try:
        import trained_fixture as tf
        wts, frames, _ = tf.train_like()
        tnet = tf.build(wts, args.precision)
        lines.append(distortion(tnet, torch.from_numpy(frames[0][0]).to(device), 9, "trained-like fixture (tests/trained_fixture.py), its first frame"))
    except Exception as e:          # the fixture is a convenience of this tool: say so and measure on what is at hand
        lines.append("  the trained-like fixture was not available (%s: %s)" % (type(e).__name__, e))
    lines.append(distortion(net, x, 9, "untrained network on the timed frame"))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
