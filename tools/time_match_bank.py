#!/usr/bin/env python3
"""Time the memory bank of appearance matching (osvos_pytorch_amd.match.bank_update / MemoryBank -> osvos_match_bank_update,
csrc/match_bank.hip) next to osvos_match_nearest of the same process, which it leaves unchanged and which is therefore the yardstick: the
update alone, the search over a bank that has grown, and the whole matcher call with a full memory next to the default matcher and the
plain forward.

    python tools/time_match_bank.py [--out profiles/match_bank_timing.txt] [--parent-lib PATH]          (needs the GPU)

The windowing of tools/time_match.py: a seeded 854x480 frame, N = 1, conv4_3 (layer 9: 60 x 107 = 6420 pixels of 512 channels) of an
untrained network under a half-and-half labelling; all loops in one process on one stream, alternating window by window; device events
around PASSES back-to-back calls; median [min .. max] of WINDOWS windows.  The update is timed in its most expensive setting: tau = 2 and
margin = -4 select every labelled row, so every call moves max_new rows (min(max_new, ring) of them).  The matcher with memory is timed
with the same thresholds after its ring has filled, so that every call pays for an update that writes memory_new rows and for a search over
all of protected + ring rows.  There is no bar: the numbers are recorded, and the only claims made from them are ratios within this run.

``--parent-lib``: a libosvos_hip.so built from the parent commit (check it out into a scratch worktree and run make in its csrc/).  It is
loaded next to this tree's library and its osvos_match_nearest is called on the same device buffers in a loop of its own, so that "the search
kernels are unchanged" is a measurement of this run: the ratio of medians and whether the [min .. max] ranges overlap are recorded.

NOT measured: batches above 1, layer 6, top-K over the grown bank, hardware counters, any accuracy.
"""
import argparse
import ctypes as C
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import networks.vgg_osvos as vo  # noqa: E402
from osvos_pytorch_amd import _lib, match  # noqa: E402
from osvos_pytorch_amd.augment import augment_frame  # noqa: E402
from time_match import H, PASSES, SLOW_PASSES, W, WARM, WINDOWS, scene, stats, window  # noqa: E402

LAYER = 9
MAX_NEW = (128, 512, 6420)
RINGS = (1, 3)               # in multiples of P
ALL = dict(tau=2.0, margin=-4.0)
MEMORY_NEW = 512


def parent_nearest(path, q, rinv, label, sim, ws):
    """a loop body that calls osvos_match_nearest of the library at `path` on the given device tensors (searched against themselves)"""
    lib = C.CDLL(path)
    res, argtypes = _lib.PROTOTYPES["osvos_match_nearest"]
    lib.osvos_match_nearest.restype, lib.osvos_match_nearest.argtypes = res, argtypes
    n, p, c = (int(v) for v in q.shape)
    ptr = [C.c_void_p(t.data_ptr()) for t in (q, rinv, q, rinv, label, sim)]

    def call():
        rc = lib.osvos_match_nearest(*ptr, None, C.c_void_p(ws.data_ptr()), n, 1, p, p, c, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--precision", default="fp32x3")
    ap.add_argument("--parent-lib", default="", help="libosvos_hip.so of the parent commit: its nearest is timed in the same process")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    net = vo.OSVOS(pretrained=0).to(device)
    net.set_precision(args.precision)
    frame = scene().to(device)
    x = augment_frame(frame, None, False, None)[0][None]

    def image():
        return augment_frame(frame, None, False, None)[0][None]

    def forward():
        with torch.no_grad():
            net.forward(image())

    mask = torch.zeros((1, H, W), device=device, dtype=torch.uint8)
    mask[:, :, :W // 2] = 1
    feat = net.forward_features(x, LAYER)[1].clone()
    _, h, w, c = (int(v) for v in feat.shape)
    p = h * w
    q, rinv = match.quantize(feat)
    q, rinv = q.view(1, p, c), rinv.view(1, p)
    label = match.cell_labels(mask, match.stride_of(LAYER)).view(1, p)
    ws = match.nearest_workspace(1, p, p, c, device)
    sim = match.nearest(q, rinv, q, rinv, label, ws=ws)
    labelled = int(((label <= 1) & (rinv > 0)).sum())
    FWD, NEAR = 0, 1
    loops = [("854x480 one test forward (augment_frame identity + net.forward)", forward, SLOW_PASSES),
             ("nearest Pr = P (%d x %d x %d), the unchanged kernel" % (p, p, c), lambda: match.nearest(q, rinv, q, rinv, label, ws=ws), PASSES)]
    parent = None
    if args.parent_lib:
        parent = len(loops)
        psim, pws = torch.empty_like(sim), torch.empty_like(ws)
        loops.append(("nearest Pr = P, the PARENT commit's build of the kernel (direct call, no wrapper)", parent_nearest(args.parent_lib, q, rinv, label, psim, pws),
                      PASSES))
        direct = len(loops)
        dsim, dws = torch.empty_like(sim), torch.empty_like(ws)
        loops.append(("nearest Pr = P, this tree's build (direct call, no wrapper)", parent_nearest(_lib.SO_PATH, q, rinv, label, dsim, dws), PASSES))
    grown = {}
    for k in RINGS:                                   # a bank that has filled: the first frame's rows, then k copies of them
        r, rr, rl = q.repeat(1, k + 1, 1), rinv.repeat(1, k + 1), label.repeat(1, k + 1)
        wk = match.nearest_workspace(1, p, (k + 1) * p, c, device)
        grown[k] = len(loops)
        loops.append(("nearest Pr = P + ring, ring = %d P (%d reference rows)" % (k, (k + 1) * p),
                      lambda r=r, rr=rr, rl=rl, wk=wk: match.nearest(q, rinv, r, rr, rl, ws=wk), PASSES))
    updates = {}
    cap = 4 * p
    for max_new in MAX_NEW:
        bank = (torch.zeros((1, cap, c), device=device, dtype=torch.int8), torch.zeros((1, cap), device=device),
                torch.full((1, cap), 255, device=device, dtype=torch.uint8), torch.zeros((1, 4), device=device, dtype=torch.int32))
        wb = match.bank_workspace(1, p, device)
        updates[max_new] = len(loops)
        loops.append(("bank update, max_new %d: %d of %d rows selected, %d rows = %d bytes moved per call (ring 3 P)"
                      % (max_new, labelled, p, min(max_new, labelled), min(max_new, labelled) * c),
                      lambda bank=bank, wb=wb, max_new=max_new: match.bank_update(q, rinv, label, sim, *bank, max_new=max_new, protected=p, ws=wb, **ALL), PASSES))
    default = match.AppearanceMatcher(net, LAYER, 4.0).set_reference(x, mask)
    memory = match.AppearanceMatcher(net, LAYER, 4.0, memory=3 * p, memory_new=MEMORY_NEW, memory_tau=ALL["tau"], memory_margin=ALL["margin"])
    memory.set_reference(x, mask)
    memory(image(), None)
    while memory._memory.rows < memory._memory.protected + memory._memory.ring:          # fill the ring: the steady state of a long sequence
        memory(image(), mask)
    DEF = len(loops)
    loops.append(("854x480 AppearanceMatcher, defaults (forward_features + quantize + nearest + fuse)", lambda: default(image()), SLOW_PASSES))
    loops.append(("854x480 AppearanceMatcher memory=3 P, memory_new=%d, ring full (+ cell_labels + update + nearest over 4 P rows)" % MEMORY_NEW,
                  lambda: memory(image(), mask), SLOW_PASSES))
    for _ in range(WARM):
        for _, fn, _ in loops:
            fn()
    times = [[] for _ in loops]
    for _ in range(WINDOWS):
        for i, (_, fn, passes) in enumerate(loops):
            times[i].append(window(fn, passes))
    med = [float(np.median(t)) for t in times]
    state = memory._memory.state.cpu().numpy()[0].tolist()
    lines = ["command: python tools/time_match_bank.py%s   (%s, torch %s, precision %s, GPU_MAX_HW_QUEUES=%s)"
             % (" --parent-lib <the parent commit's libosvos_hip.so>" if args.parent_lib else "", torch.cuda.get_device_name(0), torch.__version__, args.precision,
                os.environ.get("GPU_MAX_HW_QUEUES", "unset")),
             "batch 1, conv4_3 of an untrained network on a seeded 854x480 frame (P = %d, C = %d) under a half-and-half labelling; us per CALL through the" % (p, c),
             "Python wrapper unless a line says otherwise (every launch of the call, output allocation included), median [min .. max] of %d windows of %d"
             % (WINDOWS, PASSES),
             "calls (%d for the forward and the matchers), device events, the loops alternating in one process on one stream; 'x nearest' and 'x forward'" % SLOW_PASSES,
             "are ratios of medians within this run.  The update runs with tau = 2, margin = -4 (every labelled row selected: its most expensive setting);",
             "the matcher with memory runs with the same thresholds and a full ring, state after the run %s.  No bar is set: recorded, not gated." % (state,),
             "Not measured: batches above 1, layer 6, top-K over the grown bank, hardware counters, any accuracy."]
    for (name, _, _), t, m in zip(loops, times, med):
        lines.append("  %-118s %s   x nearest %6.3f   x forward %6.3f" % (name, stats(t), m / med[NEAR], m / med[FWD]))
    for max_new in MAX_NEW:
        m = med[updates[max_new]]
        lines.append("  update at max_new %d: %.3f of the nearest search of this run" % (max_new, m / med[NEAR]))
    for k in RINGS:
        lines.append("  nearest over P + %d P rows: %.2f x nearest over P rows (%d x the rows)" % (k, med[grown[k]] / med[NEAR], k + 1))
    lines.append("  default matcher minus forward: %.1f us; matcher with a full memory minus default matcher: %.1f us (%.3f of the forward)"
                 % (med[DEF] - med[FWD], med[DEF + 1] - med[DEF], (med[DEF + 1] - med[DEF]) / med[FWD]))
    if parent is None:
        lines.append("  the parent commit's build was not given (--parent-lib): the unchanged search kernels were NOT compared with it in this run")
    else:
        a, b = times[direct], times[parent]
        overlap = min(a) <= max(b) and min(b) <= max(a)
        lines.append("  nearest Pr = P, this tree's build / the parent commit's build, both called directly: ratio of medians %.4f; the [min .. max] ranges %s"
                     % (med[direct] / med[parent], "overlap" if overlap else "do NOT overlap"))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
