#!/usr/bin/env python3
"""Time osvos_lucid_compose_ex (csrc/lucid.hip: the lucid composition with a deformation field, an occluder and a void band) next to the
plain osvos_lucid_compose -- of this tree and, with --parent-lib, of the library built from the parent commit, called through the same
unchanged entry point in the same process -- and next to the training step the samples feed.

    python tools/time_lucid_deform.py [--parent-lib /path/to/the/parent/build/libosvos_hip.so] [--out profiles/lucid_deform_timing.txt]

The scene, the event windows and the reporting are tools/time_lucid.py's: a seeded 854x480 frame (a textured ellipse on a gradient under +-12
colour noise), sixteen parameter sets drawn once with random.seed(0) from a LucidDream with deform 0.5 on a 128-pixel lattice and an occluder in
every sample; all loops in one process on one stream, alternating window by window; device events around PASSES back-to-back calls; median
[min .. max] of WINDOWS windows.  The rows 'alone' call the library with arguments and outputs prepared once; the rows 'lucid.compose' go
through the Python wrapper (checks, output allocation, and the upload of the field).  Before anything is timed every variant's output is
compared with the plain call's where the rule says they are equal.  There is no bar: the numbers are recorded, and the only claims made from
them are ratios of the same run."""
import argparse
import ctypes as C
import os
import random
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import networks.vgg_osvos as vo  # noqa: E402
from osvos_pytorch_amd import _lib, lucid  # noqa: E402
from osvos_pytorch_amd.augment import MEANVAL  # noqa: E402
from osvos_pytorch_amd.train_common import TrainLoop, make_sgd  # noqa: E402
from time_lucid import H, PASSES, SLOW_PASSES, W, WARM, WINDOWS, scene, stats, window  # noqa: E402

CELL, BAND = 128, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--precision", default="fp32x3")
    ap.add_argument("--parent-lib", default="", help="libosvos_hip.so built from the parent commit (its osvos_lucid_compose is timed in this run)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    random.seed(0)
    net = vo.OSVOS(pretrained=0).to(device)
    net.set_precision(args.precision)
    loop = TrainLoop(net, make_sgd(net, "online"), mode="online", n_ave_grad=1)
    frame, mask = [t.to(device) for t in scene()]
    dream = lucid.LucidDream(frame, mask, deform=0.5, deform_cell=CELL, occlude=1.0)
    draws = [dream.draw() for _ in range(16)]
    M, T = np.asarray([d[0] for d in draws], np.float64), np.asarray([d[1] for d in draws], np.int32)
    D, O = np.asarray([d[2] for d in draws], np.int16), np.asarray([d[3] for d in draws], np.int32)
    assert (O[:, 2] > 0).all() and (O[:, 3] > 0).all() and D.any()
    d_dev = torch.from_numpy(D).to(device)
    vp, mean, stream = C.c_void_p, (C.c_float * 3)(*MEANVAL), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(_lib.lib().osvos_lucid_compose_ex_ws_bytes(16, H, W, 16) // 8, device=device, dtype=torch.int64)
    parent = None
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        assert not hasattr(parent, "osvos_lucid_compose_ex"), "--parent-lib already has osvos_lucid_compose_ex: not the parent commit's build"
        parent.osvos_lucid_compose.restype, parent.osvos_lucid_compose.argtypes = _lib.PROTOTYPES["osvos_lucid_compose"]
    outs = {}

    def plain(fn, n, name):
        """osvos_lucid_compose of a library alone"""
        out_img, out_gt = torch.empty((n, 3, H, W), device=device), torch.empty((n, 1, H, W), device=device)
        a = (vp(frame.data_ptr()), vp(mask.data_ptr()), vp(dream.bg.data_ptr()), vp(M.ctypes.data), vp(T.ctypes.data), mean, vp(out_img.data_ptr()),
             vp(out_gt.data_ptr()), n, H, W, stream)
        outs[name] = (out_img, out_gt)

        def call():
            assert fn(*a) == 0
        return call

    def ex(n, name, deform=False, occlude=False, band=0):
        """osvos_lucid_compose_ex alone"""
        out_img, out_gt = torch.empty((n, 3, H, W), device=device), torch.empty((n, 1, H, W), device=device)
        a = (vp(frame.data_ptr()), vp(mask.data_ptr()), vp(dream.bg.data_ptr()), vp(M.ctypes.data), vp(T.ctypes.data),
             vp(O.ctypes.data) if occlude else None, vp(d_dev.data_ptr()) if deform else None, CELL, band, mean, vp(out_img.data_ptr()),
             vp(out_gt.data_ptr()), n, H, W, vp(ws.data_ptr()) if band else None, stream)
        outs[name] = (out_img, out_gt)
        fn = _lib.lib().osvos_lucid_compose_ex

        def call():
            assert fn(*a) == 0
        return call

    sample = {}

    def step():
        loop.micro_batch(sample["image"].detach().requires_grad_(), sample["gt"], void_labels=True)

    def wrapped_full():
        return lucid.compose(frame, mask, dream.bg, M[:1], T[:1], occluders=O[:1], field=D[:1], cell=CELL, band=BAND, ws=ws)
    sample["image"], sample["gt"] = [t.clone() for t in wrapped_full()]

    this = _lib.lib().osvos_lucid_compose
    loops = [("854x480 fp32x3 training step on a full sample (TrainLoop.micro_batch, void labels, one optimizer step)", step, SLOW_PASSES)]
    if parent is not None:
        loops += [("osvos_lucid_compose alone, N = 16, THE PARENT COMMIT'S BUILD", plain(parent.osvos_lucid_compose, 16, "parent16"), PASSES),
                  ("osvos_lucid_compose alone, N = 1, THE PARENT COMMIT'S BUILD", plain(parent.osvos_lucid_compose, 1, "parent1"), PASSES)]
    loops += [("osvos_lucid_compose alone, N = 16", plain(this, 16, "plain16"), PASSES),
              ("osvos_lucid_compose alone, N = 1", plain(this, 1, "plain1"), PASSES),
              ("osvos_lucid_compose_ex alone, N = 16, everything off", ex(16, "off16"), PASSES),
              ("osvos_lucid_compose_ex alone, N = 16, deformation only (cell %d)" % CELL, ex(16, "deform16", deform=True), PASSES),
              ("osvos_lucid_compose_ex alone, N = 16, occluder only", ex(16, "occ16", occlude=True), PASSES),
              ("osvos_lucid_compose_ex alone, N = 16, band %d only (two launches)" % BAND, ex(16, "band16", band=BAND), PASSES),
              ("osvos_lucid_compose_ex alone, N = 16, band 16 only (two launches)", ex(16, "wide16", band=16), PASSES),
              ("osvos_lucid_compose_ex alone, N = 16, all three (band %d)" % BAND, ex(16, "full16", True, True, BAND), PASSES),
              ("osvos_lucid_compose_ex alone, N = 1, all three (band %d)" % BAND, ex(1, "full1", True, True, BAND), PASSES),
              ("lucid.compose, N = 1, as before", lambda: lucid.compose(frame, mask, dream.bg, M[:1], T[:1]), PASSES),
              ("lucid.compose, N = 1, all three (band %d; the field uploaded per call)" % BAND, wrapped_full, PASSES)]
    names = [l[0] for l in loops]
    for _ in range(WARM):
        for _, fn, _ in loops:
            fn()
    torch.cuda.synchronize()
    # what the rule says is equal, is equal: before anything is timed
    same = lambda a, b: torch.equal(outs[a][0].view(torch.int32), outs[b][0].view(torch.int32)) and torch.equal(outs[a][1], outs[b][1])  # noqa: E731
    assert same("plain16", "off16")
    if parent is not None:
        assert same("plain16", "parent16") and same("plain1", "parent1")
    assert torch.equal(outs["band16"][0], outs["plain16"][0]) and torch.equal(outs["band16"][1] != 0, (outs["band16"][1] < 0) | (outs["plain16"][1] != 0))
    assert torch.equal(outs["full1"][0][0], sample["image"][0]) and torch.equal(outs["full1"][1][0], sample["gt"][0])
    void = float((outs["full16"][1] < 0).float().mean())
    times = [[] for _ in loops]
    for _ in range(WINDOWS):
        for i, (_, fn, passes) in enumerate(loops):
            times[i].append(window(fn, passes))
    med = {n: float(np.median(t)) for n, t in zip(names, times)}
    span = {n: (min(t), max(t)) for n, t in zip(names, times)}
    lines = ["command: python tools/time_lucid_deform.py%s   (%s, torch %s, precision %s, GPU_MAX_HW_QUEUES=%s)"
             % (" --parent-lib <the parent commit's build>" if parent is not None else "", torch.cuda.get_device_name(0), torch.__version__, args.precision,
                os.environ.get("GPU_MAX_HW_QUEUES", "unset")),
             "the scene of tools/time_lucid.py, 16 parameter sets drawn with random.seed(0) from LucidDream(deform=0.5, deform_cell=%d, occlude=1.0);" % CELL,
             "us per CALL, median [min .. max] of %d windows of %d calls (%d for the training step), device events, the loops alternating in one"
             % (WINDOWS, PASSES, SLOW_PASSES),
             "process on one stream; 'x step' is the ratio of medians to the training step of this run.  %.2f %% of the labels of the full samples"
             % (100 * void),
             "are void.  Outputs were compared before timing: everything off = the plain call%s, bit for bit.  No bar is set: recorded, not gated."
             % (" = the parent build's call" if parent is not None else "")]
    for (name, _, _), t in zip(loops, times):
        lines.append("  %-100s %s   x step %7.4f" % (name, stats(t), np.median(t) / med[names[0]]))
    per = lambda frag: med[next(n for n in names if n.endswith(frag) or frag in n and "_ex" in n and "N = 16" in n)] / 16.0  # noqa: E731
    lines.append("  per sample at N = 16: plain %.1f us, everything off %.1f us, deformation %.1f us, occluder %.1f us, band %d %.1f us, band 16 %.1f us, "
                 "all three %.1f us" % (per("osvos_lucid_compose alone, N = 16"), per("everything off"), per("deformation only"), per("occluder only"), BAND,
                                        per("band %d only" % BAND), per("band 16 only"), per("all three")))
    if parent is not None:
        for n in (16, 1):
            a, b = "osvos_lucid_compose alone, N = %d, THE PARENT COMMIT'S BUILD" % n, "osvos_lucid_compose alone, N = %d" % n
            overlap = span[a][0] <= span[b][1] and span[b][0] <= span[a][1]
            lines.append("  (a) the plain entry point against the parent commit's build, N = %d: ratio of medians %.3f; the window ranges %s"
                         % (n, med[b] / med[a], "overlap" if overlap else "DO NOT overlap"))
    full, before = names[-1], names[-2]
    lines.append("  (b) a full sample through the wrapper: %.4f of the training step (as before: %.4f); the launches alone at N = 1: %.4f"
                 % (med[full] / med[names[0]], med[before] / med[names[0]], med["osvos_lucid_compose_ex alone, N = 1, all three (band %d)" % BAND] / med[names[0]]))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
