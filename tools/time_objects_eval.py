#!/usr/bin/env python3
"""Time the multi-object result path (results.merge_objects + results.MultiObjectEvaluator.add: osvos_merge_objects, osvos_labels_jf_counts)
next to what the single-object entry points need for the same answer: torch max / compare ops that turn the K logit stacks into K pairs
of float masks, then K osvos_mask_jf_counts calls.

    python tools/time_objects_eval.py [--out profiles/objects_eval.txt]          (needs the GPU)

Input: a synthetic 854x480 sequence of 64 frames with K = 3 objects -- three ellipses that drift against their ground truth, under noisy
logits.  Both paths run in the same process on the same tensors, alternating; times are device events around 20 back-to-back passes over
the sequence after 3 warm-up passes, median [min .. max] of 7 such windows, reported per frame.  The two count tables must be equal.
"""
import argparse
import ctypes as C
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from osvos_pytorch_amd import _lib, results  # noqa: E402

PASSES, WARM, WINDOWS = 20, 3, 7


def sequence(device, frames, k, h, w):
    """logits [K, F, H, W] and uint8 ground-truth labels [F, H, W]"""
    gen = torch.Generator().manual_seed(11)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    gt = torch.zeros(frames, h, w, dtype=torch.uint8)
    logits = torch.empty(k, frames, h, w)
    for j in range(k):
        cx = (j + 0.5) / k
        for f in range(frames):
            d_gt = ((yy - 0.5 * h) / (0.3 * h)) ** 2 + ((xx - cx * w - 0.3 * f) / (0.4 * w / k)) ** 2
            d_pr = ((yy - 0.5 * h - 0.1 * f) / (0.3 * h)) ** 2 + ((xx - cx * w - 0.4 * f) / (0.42 * w / k)) ** 2
            gt[f][d_gt <= 1] = j + 1
            logits[j, f] = (1.0 - d_pr) * 4.0 + 0.3 * torch.randn(h, w, generator=gen)
    return logits.to(device).contiguous(), gt.to(device).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--objects", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    device = torch.device("cuda:0")
    f, k, h, w = args.frames, args.objects, 480, 854
    logits, gt = sequence(device, f, k, h, w)
    r = results.boundary_radius(h, w)
    l = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(l.osvos_boundary_ws_bytes(f, h, w) // 8, device=device, dtype=torch.int64)
    old_counts = torch.empty((k, f, 6), device=device, dtype=torch.int64)
    ev = [None]

    def new_path():
        ev[0] = results.MultiObjectEvaluator(k)
        ev[0].add(results.merge_objects(logits), gt)

    def old_path():
        m, idx = logits.max(0)
        lab = torch.where(m > 0, idx + 1, torch.zeros_like(idx))
        for j in range(k):
            x = (lab == j + 1).float() * 2 - 1
            g = (gt == j + 1).float()
            _lib.check(l.osvos_mask_jf_counts(C.c_void_p(x.data_ptr()), C.c_void_p(g.data_ptr()), C.c_void_p(ws.data_ptr()),
                                              C.c_void_p(old_counts[j].data_ptr()), f, h, w, 0.0, r, 0, st))

    def window_us(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(PASSES):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / (PASSES * f)

    for _ in range(WARM):
        new_path()
        old_path()
    torch.cuda.synchronize()
    tn, to = [], []
    for _ in range(WINDOWS):
        tn.append(window_us(new_path))
        to.append(window_us(old_path))
    torch.cuda.synchronize()
    new_counts = ev[0]._table[:f].cpu().numpy()
    same = np.array_equal(new_counts, old_counts.cpu().numpy().transpose(1, 0, 2))
    s = ev[0].summary()
    lines = ["command: python tools/time_objects_eval.py   (%s, torch %s)" % (torch.cuda.get_device_name(0), torch.__version__),
             "%dx%d, K = %d objects, %d frames, r = %d; us per FRAME, device events around %d passes over the sequence, median [min .. max] of %d windows,"
             % (w, h, k, f, r, PASSES, WINDOWS), "the two paths alternating in one process, one stream.  What each pass includes besides its kernels: the new path",
             "builds a MultiObjectEvaluator per pass (a torch.zeros count table, a workspace and the label tensor from the caching allocator); the old",
             "path reuses a preallocated workspace and count table but allocates its torch temporaries (max, where, K x compare / float) per pass.",
             "  merge_objects + MultiObjectEvaluator.add (osvos_merge_objects, memset + labels_pack_kernel + jf_match_kernel) %8.2f [%7.2f .. %7.2f]"
             % (np.median(tn), min(tn), max(tn)),
             "  torch max / where / K x (compare, float) + K x osvos_mask_jf_counts (what the parent commit needs)            %8.2f [%7.2f .. %7.2f]"
             % (np.median(to), min(to), max(to)),
             "  ratio old / new %.2f;  count tables equal: %s;  sequence J %.4f F %.4f" % (np.median(to) / np.median(tn), same, s["J"], s["F"])]
    text = "\n".join(lines) + "\n"
    print(text)
    assert same, "the two paths disagree"
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
