"""The pipelined K loop of the f32x3 convolution (tiles 10, 12, 14 with the pre-split pack) against the single-buffered loop it replaces
(OSVOS_X3_PIPE=0): bit for bit, on the wide layer shapes of the 854x480 batch-1 step, forward and data gradient, plain grid and stream-K
(with several tiles per persistent workgroup), the fused pool forward, the ReLU mask, a channel stride, an odd frame, and a whole training
step of the network (split-K data gradients, stream-K, fused epilogues).  The switch is read once per process, so each arm runs in a
child process of its own."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (N, H, W, Cin, Cout) of the 3x3 convolutions at 854x480 batch 1 whose forward or data gradient runs on tiles 10 / 12 / 14
WIDE = [
    (1, 480, 854, 64, 64),       # conv1_2
    (1, 240, 427, 64, 128),      # conv2_1
    (1, 240, 427, 128, 128),     # conv2_2
    (1, 120, 214, 128, 256),     # conv3_1
    (1, 120, 214, 256, 256),     # conv3_2 / 3_3
    (1, 60, 107, 256, 512),      # conv4_1
    (1, 60, 107, 512, 512),      # conv4_2 / 4_3
    (1, 30, 54, 512, 512),       # conv5_x
    (1, 37, 53, 64, 128),        # an odd frame
]

CHILD = r"""
import os, sys, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from osvos_pytorch_amd import ops
from relu_mask_cases import post_relu_mask
shapes = eval(sys.argv[2])
out = {}
def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().cuda()
for k, (n, h, w, cin, cout) in enumerate(shapes):
    g = torch.Generator().manual_seed(100 + k)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    b = torch.randn(cout, generator=g)
    dy = torch.randn(n, cout, h, w, generator=g)
    m = post_relu_mask((n, cin, h, w), 100 + k, torch.float32)      # a real post-ReLU operand: exact zeros, -0.0, dead blocks
    xg, pk3, dpk3 = nhwc(x), ops.pack_x3(wt.cuda()), ops.pack_x3(wt.cuda(), dgrad=True)
    for t in (-1, 10, 12, 14):
        out["fwd", k, t] = ops.conv3x3_x3(xg, pk3, b.cuda(), cout, relu=True, tile=t).cpu()
        out["dgrad", k, t] = ops.conv3x3_x3(nhwc(dy), dpk3, None, cin, mask=nhwc(m), tile=t).cpu()
    out["stride", k] = ops.conv3x3_x3(xg, pk3, b.cuda(), cout, relu=False, y_cs=cout + 8).cpu()
    for t in (10, 12, 14):
        th, tw, bn = {10: (8, 32, 128), 12: (8, 32, 64), 14: (16, 16, 64)}[t]
        units = lambda k_, m_: n * -(-h // th) * -(-w // tw) * -(-(-(-m_ // 32) * 32) // bn) * (k_ // 16)
        for grid in (0, 37, 256):       # automatic, few persistent workgroups (several tiles each), one per CU
            if grid > min(units(cin, cout), units(cout, cin)):
                continue
            y, p = ops.conv3x3_x3_streamk(xg, pk3, b.cuda(), cout, relu=True, tile=t, grid=grid, want_pooled=True)
            out["sk", k, t, grid] = y.cpu()
            out["skpool", k, t, grid] = p.cpu()
            out["skdgrad", k, t, grid] = ops.conv3x3_x3_streamk(nhwc(dy), dpk3, None, cin, mask=nhwc(m), tile=t, grid=grid).cpu()
torch.cuda.synchronize()
torch.save(out, sys.argv[3])
"""

NET_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
import bench
from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
net, x, gt = bench.synth_problem(1, 480, 854, torch.device("cuda:0"), seed=0)
net.set_precision("fp32x3")
outs = net.forward(x)
loss = sum(cbce(o, gt, size_average=False) for o in outs)
loss.backward()
torch.cuda.synchronize()
res = {"out%d" % i: o.detach().cpu() for i, o in enumerate(outs)}
res.update({"grad." + k: p.grad.detach().cpu() for k, p in net.named_parameters() if p.grad is not None})
torch.save(res, sys.argv[2])
"""


def _run(code, args, pipe, tmp_path, tag):
    path = str(tmp_path / ("%s_pipe%d.pt" % (tag, pipe)))
    env = dict(os.environ, OSVOS_X3_PIPE=str(pipe))
    r = subprocess.run([sys.executable, "-c", code, REPO] + args + [path], env=env, cwd=REPO, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (pipe, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return torch.load(path)


def _same(old, new):
    assert old.keys() == new.keys()
    bad = [k for k in old if not torch.equal(old[k], new[k])]
    assert not bad, bad[:10]


@pytest.mark.parametrize("shapes", [WIDE[:4], WIDE[4:]], ids=["shallow", "deep"])
def test_x3_pipelined_loop_is_bit_identical_per_layer(shapes, tmp_path):
    old = _run(CHILD, [repr(shapes)], 0, tmp_path, "ops")
    new = _run(CHILD, [repr(shapes)], 1, tmp_path, "ops")
    _same(old, new)
    assert all(torch.isfinite(v).all() for v in new.values())


def test_x3_pipelined_loop_is_bit_identical_network_step(tmp_path):
    old = _run(NET_CHILD, [], 0, tmp_path, "net")
    new = _run(NET_CHILD, [], 1, tmp_path, "net")
    _same(old, new)
    assert len([k for k in new if k.startswith("grad.")]) > 30
