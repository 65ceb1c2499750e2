#!/usr/bin/env python3
"""The ordered kernel launches of one training micro-batch, for comparing two builds launch by launch (host-side refactors of the launchers
must leave the list unchanged: kernel names carry the template arguments, so an equal list means every layer got the kernel it got before).

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/launch_list.py run --precision fp32x3 [--repo OTHER_CHECKOUT]
    python tools/launch_list.py report DIR > list.txt        # one line per launch, in dispatch order: kernel | grid | workgroup | LDS bytes
    python tools/launch_list.py report DIR --after sgd       # ... of any traced program, from the first launch whose kernel name holds "sgd" on

`run` does ONE forward + loss + backward of the network at 1 x 480 x 854 after the packs are written (no warm-up pass: every launch counts)."""
import argparse
import csv
import glob
import os
import sys


def run(args):
    repo = os.path.abspath(args.repo or os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    sys.path.insert(0, repo)
    import torch
    import networks.vgg_osvos as vo
    from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
    from oracle import synth
    wts, x, m = synth.make_weights(1), synth.make_frame(1, args.height, args.width, 3), synth.make_mask(1, args.height, args.width, 3)
    net = vo.OSVOS(pretrained=0)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in wts.items()})
    net = net.to("cuda:0").set_precision(args.precision)
    outs = net.forward(torch.from_numpy(x).to("cuda:0"))
    loss = cbce(outs[-1], torch.from_numpy(m).to("cuda:0"), size_average=False)
    loss.backward()
    torch.cuda.synchronize()
    print("launch_list: %s loss %.6f" % (args.precision, loss.item()))


def report(args):
    rows = []
    for f in glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            r = {k.lower(): v for k, v in r.items()}
            rows.append((int(r["dispatch_id"]), r["kernel_name"], "x".join(r["grid_size_" + a] for a in "xyz"),
                         "x".join(r["workgroup_size_" + a] for a in "xyz"), r["lds_block_size"]))
    assert rows, "no kernel trace under " + args.dir
    rows.sort()
    if args.after:
        rows = rows[min(i for i, r in enumerate(rows) if args.after in r[1]) + 1:]
    for _, name, grid, wg, lds in rows:
        print("%s | %s | %s | %s" % (name, grid, wg, lds))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--precision", default="fp32x3")
    r.add_argument("--height", type=int, default=480)
    r.add_argument("--width", type=int, default=854)
    r.add_argument("--repo", default=None, help="the checkout whose package runs (default: this one)")
    p = sub.add_parser("report")
    p.add_argument("dir")
    p.add_argument("--after", default="", help="leave out everything up to and including the first launch whose kernel name contains this")
    a = ap.parse_args()
    run(a) if a.cmd == "run" else report(a)
