#!/usr/bin/env python3
"""Time the stages of interactive scribbles (osvos_pytorch_amd.scribble -> osvos_scribble_raster, osvos_mask_thin; csrc/scribble.hip) at
854x480, all in one run: the raster at 64 and 1024 segments of radius 3; the thinning of the synthetic frame's annotation (a filled ellipse:
many iterations) and of a thin error ring (few), each on the LDS-resident path 1 and the global path 2; ``error_scribbles`` as a whole; one
session sample (two ``augment_frame`` calls and the glue) next to a single ``augment_frame`` call; and that run's test forward, so that every
figure is also a fraction of it.

    python tools/time_scribble.py [--out profiles/scribble_timing.txt] [--parent-lib PATH]          (needs the GPU)

``--parent-lib`` names a shared library built from the PARENT commit's csrc/components.hip (with csrc/errors.cpp): its osvos_mask_components,
a kernel this change leaves untouched, is loaded into this process and timed against this tree's through the same ctypes path, window by
window.  The two must be level: the window ranges overlap, and the output says whether they do.

The windowing of tools/time_match.py: all loops in one process on one stream, alternating window by window; device events around PASSES
back-to-back calls; median [min .. max] of WINDOWS windows.  There is no bar: the numbers are recorded, and ``thin``'s automatic choice of
path (path = 0) follows what this run shows; the rule and the numbers behind it are written at the end of the output.

NOT measured: other frame sizes, batches above 1, hardware counters, any accuracy.
"""
import argparse
import ctypes as C
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tools"))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import networks.vgg_osvos as vo  # noqa: E402
from osvos_pytorch_amd import _lib, scribble  # noqa: E402
from osvos_pytorch_amd.augment import DeviceAugment, augment_frame  # noqa: E402
from time_match import H, PASSES, SLOW_PASSES, W, WARM, WINDOWS, scene, stats, window  # noqa: E402


def ellipse(ry, rx, cy=0.5 * H, cx=0.5 * W):
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1


def direct_components(lib, x, labels, area, st, ws):
    """osvos_mask_components of ``lib`` through ctypes, the pointers made once -> a callable"""
    n, h, w = (int(v) for v in x.shape)
    fn = lib.osvos_mask_components
    fn.restype, fn.argtypes = _lib.PROTOTYPES["osvos_mask_components"]
    ptrs = [C.c_void_p(t.data_ptr()) for t in (x, labels, area, st, ws)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        rc = fn(*ptrs, n, h, w, 0.0, 8, stream)
        assert rc == 0, rc
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--precision", default="fp32x3")
    ap.add_argument("--parent-lib", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    net = vo.OSVOS(pretrained=0).to(device)
    net.set_precision(args.precision)
    frame = scene().to(device)

    def forward():
        with torch.no_grad():
            net.forward(augment_frame(frame, None, False, None)[0][None])

    rng = np.random.RandomState(0)
    tables = {}
    for m in (64, 1024):          # strokes of about 40 pixels a segment, as a polyline's pieces are
        a = np.stack([rng.randint(0, W, m), rng.randint(0, H, m)], axis=1)
        b = np.clip(a + rng.randint(-40, 41, (m, 2)), 0, [W - 1, H - 1])
        tables[m] = torch.from_numpy(np.concatenate([a, b, rng.randint(0, 3, (m, 1)), np.zeros((m, 1), dtype=np.int64)], axis=1).astype(np.int32)).to(device)
    out_map = torch.empty((1, H, W), device=device, dtype=torch.uint8)
    gt = torch.from_numpy(ellipse(0.25 * H, 0.25 * W).astype(np.uint8)).to(device)[None]            # train_online.py's synthetic annotation
    pred = torch.from_numpy(ellipse(0.25 * H + 6, 0.25 * W + 6, 0.5 * H + 3, 0.5 * W + 4).astype(np.uint8)).to(device)[None]
    ring = (pred != gt).to(torch.uint8)                                                              # a thin error ring
    skel = torch.empty((1, H, W), device=device, dtype=torch.uint8)
    info = {}
    masks = (("ellipse", gt, 64), ("ellipse", gt, 512), ("ring", ring, 64))            # (the first interaction thins with max_iters 512)
    for name, mask, iters in masks:
        for path in (1, 2):
            s, i = scribble.thin(mask, iters, path)
            info[name, iters, path] = (i.cpu().tolist()[0], int(s.sum()))
        assert info[name, iters, 1] == info[name, iters, 2], (name, info)
    session = scribble.InteractiveSession(None, None, [frame], 1, augment=DeviceAugment(rots=(-30, 30), scales=(.75, 1.25)), loop=object())
    session.add(0, scribble.initial_scribbles(gt)[0])
    lab = gt[0] * 255

    loops = [("854x480 one test forward (augment_frame identity + net.forward)", forward, SLOW_PASSES)]
    index = {}

    def add(key, name, fn, passes=PASSES):
        index[key] = len(loops)
        loops.append((name, fn, passes))

    for m in (64, 1024):
        add(("raster", m), "raster, M = %d segments, radius 3" % m, lambda t=tables[m]: scribble.raster_segments(t, (H, W), 3, 1, out=out_map))
    for name, mask, iters in masks:
        for path in (1, 2):
            i = info[name, iters, path]
            add(("thin", name, iters, path), "thin, %s (%d iterations run, flag %d, %d skeleton pixels), path %d, max_iters %d" % (name, i[0][0], i[0][1], i[1], path, iters),
                lambda mask=mask, path=path, iters=iters: scribble.thin(mask, iters, path, out=skel), PASSES if iters == 64 else SLOW_PASSES)
    add("error", "error_scribbles (components + thin + distance map + glue) on the ring", lambda: scribble.error_scribbles(pred, gt), SLOW_PASSES)
    add("initial", "initial_scribbles (two values; one read-back) on the ellipse", lambda: scribble.initial_scribbles(gt), SLOW_PASSES)
    add("sample", "one session sample (training_planes + draw + 2 augment_frame + label)", lambda: session.sample(0))
    add("augment", "one augment_frame call with a label, a drawn warp", lambda: augment_frame(frame, lab, *session.augment.draw()))

    x = torch.where(gt != 0, 1.0, -1.0).contiguous()
    labels, area = torch.empty((1, H, W), device=device, dtype=torch.int32), torch.empty((1, H, W), device=device, dtype=torch.int32)
    st = torch.empty((1, 4), device=device, dtype=torch.int64)
    ws = torch.empty(_lib.lib().osvos_components_ws_bytes(1, H, W), device=device, dtype=torch.uint8)
    add("direct", "osvos_mask_components of this tree, direct ctypes call (the untouched control)", direct_components(_lib.lib(), x, labels, area, st, ws))
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        labels_p = torch.empty_like(labels)
        add("parent", "osvos_mask_components of the parent commit's build, direct ctypes call", direct_components(parent, x, labels_p, area, st, ws))
    for _ in range(WARM):
        for _, fn, _ in loops:
            fn()
    if args.parent_lib:
        torch.cuda.synchronize()
        assert torch.equal(labels, labels_p), "the parent's components give other labels"
    times = [[] for _ in loops]
    for _ in range(WINDOWS):
        for i, (_, fn, passes) in enumerate(loops):
            times[i].append(window(fn, passes))
    med = [float(np.median(t)) for t in times]
    lines = ["command: python tools/time_scribble.py%s   (%s, torch %s, precision %s, GPU_MAX_HW_QUEUES=%s)"
             % (" --parent-lib <the parent commit's csrc/components.hip>" if args.parent_lib else "", torch.cuda.get_device_name(0), torch.__version__,
                args.precision, os.environ.get("GPU_MAX_HW_QUEUES", "unset")),
             "batch 1 at 854x480; us per CALL through the Python wrapper (every launch of the call, allocations included; the two 'direct' loops through",
             "ctypes alone), median [min .. max] of %d windows of %d calls (%d for the forward and the two annotator calls), device events, the loops" % (WINDOWS, PASSES, SLOW_PASSES),
             "alternating in one process on one stream; 'x forward' is the ratio of medians to the test forward of this run.  No bar is set: recorded,",
             "not gated.  Not measured: other frame sizes, batches above 1, hardware counters, any accuracy."]
    for (name, _, _), t, m in zip(loops, times, med):
        lines.append("  %-100s %s   x forward %7.4f" % (name, stats(t), m / med[0]))
    lines.append("  the second warp of a session sample: sample minus one augment_frame call = %.1f us (%.4f of the forward)"
                 % (med[index["sample"]] - med[index["augment"]], (med[index["sample"]] - med[index["augment"]]) / med[0]))
    what = ["%s at max_iters %d" % (n, it) for n, _, it in masks]
    p1 = [med[index["thin", n, it, 1]] for n, _, it in masks]
    p2 = [med[index["thin", n, it, 2]] for n, _, it in masks]
    lines.append("  thinning, path 1 against path 2: %s; path 2 enqueues max_iters launches" % "; ".join("%s %.1f vs %.1f us" % (w, a, b) for w, a, b in zip(what, p1, p2)))
    lines.append("  whatever the mask holds (%.1f us a launch here), path 1 stops at convergence but runs a frame on one compute unit." % (p2[0] / 64.0))
    won = [w for w, a, b in zip(what, p1, p2) if a <= b]
    lost = ["%s (%.2f x)" % (w, a / b) for w, a, b in zip(what, p1, p2) if a > b]
    lines.append("  The rule of path = 0 (csrc/scribble.hip): path 1 whenever the frame's plane fits in LDS, else path 2.  In this run path 1 is the faster one on: %s;"
                 % (", ".join(won) or "nothing"))
    lines.append("  the slower one on: %s.  (A run that max_iters cuts short leaves a blob, not a stroke: the callers that want strokes thin to the end.)"
                 % (", ".join(lost) or "nothing"))
    if args.parent_lib:
        a, b = times[index["direct"]], times[index["parent"]]
        level = min(a) <= max(b) and min(b) <= max(a)
        lines.append("  no regression of the untouched labelling: this tree %s, the parent's build %s -- the window ranges %s; the two give the same labels"
                     % (stats(a).strip(), stats(b).strip(), "OVERLAP: level" if level else "DO NOT OVERLAP"))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
