#!/usr/bin/env python3
"""sha256 of everything the whole-network calls produce, for comparing two builds bit for bit (a host-side refactor of the network calls must
leave every hash unchanged: nothing may reorder a sum).

    python tools/net_bits.py [--repo OTHER_CHECKOUT] [--precisions fp32,bf16,..] > bits.txt

Every precision x {diagonal, dense (generic head)} deconvolution weights (tests/head_cases.apply_weight_kind) x frames 2x48x64 and 1x33x47 (odd
sides: ceil-mode pools, ragged tiles), seeded from oracle.synth.calibrated_problem.  Per case: the five logit maps of a training forward, of a
torch.no_grad() forward, forward_features(layer=9)'s tensor, all parameter gradients and dx of one backward of the summed five losses, then the
gradients after a second micro-batch accumulated in place, and after a third with the deferred join (join_backward)."""
import argparse
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--repo", default=None, help="the checkout whose package runs (default: this one)")
ap.add_argument("--precisions", default="fp32,bf16,fp32x3,fp32x2,fp32x3b2,fp32h2,fp32x3h2,bf16w2")
args = ap.parse_args()
repo = os.path.abspath(args.repo or os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [repo, os.path.join(repo, "tests")]
import torch  # noqa: E402
import networks.vgg_osvos as vo  # noqa: E402
from head_cases import apply_weight_kind  # noqa: E402
from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce  # noqa: E402
from oracle import synth  # noqa: E402


def sha(tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is None:
            h.update(b"none")
            continue
        t = t.detach().contiguous()
        h.update(str((tuple(t.shape), t.dtype)).encode())
        h.update(t.view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def grads(net, x):
    return [p.grad for p in net.parameters()] + [x.grad]


def step(net, x, m):
    outs = net.forward(x)
    sum(cbce(o, m, size_average=False) for o in outs).backward()
    return outs


for precision in args.precisions.split(","):
    for kind in ("diagonal", "dense"):
        for n, h, w in ((2, 48, 64), (1, 33, 47)):
            tag = "%-8s %-8s %dx%dx%d" % (precision, kind, n, h, w)
            wts, x_np, m_np = synth.calibrated_problem(n, h, w, seed=3)
            _, x2_np, m2_np = synth.calibrated_problem(n, h, w, seed=4)
            net = vo.OSVOS(pretrained=0)
            net.load_state_dict({k: torch.from_numpy(v) for k, v in apply_weight_kind(wts, kind).items()})
            net = net.to("cuda:0").set_precision(precision)
            x, m = torch.from_numpy(x_np).to("cuda:0").requires_grad_(), torch.from_numpy(m_np).to("cuda:0")
            x2, m2 = torch.from_numpy(x2_np).to("cuda:0").requires_grad_(), torch.from_numpy(m2_np).to("cuda:0")
            outs = step(net, x, m)
            torch.cuda.synchronize()
            print(tag, "train_forward", sha(outs))
            print(tag, "backward     ", sha(grads(net, x)), "(%d gradients)" % sum(g is not None for g in grads(net, x)))
            with torch.no_grad():
                print(tag, "no_grad      ", sha(net.forward(x.detach())))
                o, feat, fmt = net.forward_features(x.detach(), layer=9)
            print(tag, "features     ", sha(o), sha([feat]), "format", fmt)
            net.set_inplace_grad_accumulation(True)
            step(net, x2, m2)
            torch.cuda.synchronize()
            print(tag, "accumulated  ", sha(grads(net, x2)))
            net.set_deferred_backward_join(True)
            step(net, x, m)
            net.join_backward()
            torch.cuda.synchronize()
            print(tag, "deferred_join", sha(grads(net, x)))
print("net_bits: done")
