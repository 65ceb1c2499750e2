"""The early barrier of the pipelined f32x3 K loop (conv3x3_f32x3.hip, PIPE = 1: the barrier that opens tap row j + 1 sits in row j's last
step, the next row's first fragments are read in front of that step's MFMAs, the weight DMA leads the prologue) against the single-buffered
loop (OSVOS_X3_PIPE=0, untouched code that test_gpu_ops.py holds to float64): bit for bit, on the smallest shapes at which the new schedule
can go wrong.

  * segment lengths: K = 16, 32, 48, 64 reduction channels = 1, 2, 3, 4 chunks (no next row after the third; no chunk kc + 2; an odd and an
    even chunk count for the fragment sets across the chunk boundary), tiles 10 (128 couts), 12 and 14 (64 couts) forced, frame 1 x 19 x 37
    (several ragged tiles per dimension), forward with bias + ReLU and the data gradient under a post-ReLU mask (relu_mask_cases.py)
  * stream-K with 5 and 7 persistent workgroups on the same shapes: several segments per workgroup, segments of one chunk, segments that do
    not start at chunk 0; the fused pool forward on an even frame (1 x 16 x 64); the masked data gradient
  * split-K: ops.conv3x3_splitk(ksplit = 3, F32_X3) at K = 64 and 48.  Through this entry point the convolution takes the fp32 pack, i.e. the
    un-pipelined kernel in BOTH arms: the case pins that the switch leaves that path alone.  K segments of the pipelined loop that do not start
    at chunk 0 are what the stream-K cases above run (and the split-K data gradients of test_gpu_x3_pipeline.py's network step).
  * one channel stride, y_cs = Cout + 8

The switch is read once per process, so each arm runs in a child process of its own; one pair of children covers every case."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import os, sys, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from osvos_pytorch_amd import ops
from osvos_pytorch_amd._lib import F32_X3
from relu_mask_cases import post_relu_mask
out = {}
def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().cuda()
TILES = {10: (8, 32, 128), 12: (8, 32, 64), 14: (16, 16, 64)}      # tile id: (tile height, tile width, couts per tile)
def units(t, h, w, k, m):
    th, tw, bn = TILES[t]
    return -(-h // th) * -(-w // tw) * -(-m // bn) * (k // 16)
def problem(seed, h, w, k, m):
    # forward layer k -> m channels and the data gradient of a layer m -> k channels: both reduce over k channels and write m
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, k, h, w, generator=g)
    wf = torch.randn(m, k, 3, 3, generator=g) / (3 * k ** 0.5)
    wd = torch.randn(k, m, 3, 3, generator=g) / (3 * k ** 0.5)
    b = torch.randn(m, generator=g)
    dy = torch.randn(1, k, h, w, generator=g)
    mask = post_relu_mask((1, m, h, w), seed, torch.float32)
    return nhwc(x), wf.cuda(), wd.cuda(), b.cuda(), nhwc(dy), nhwc(mask)
H, W = 19, 37
for t in (10, 12, 14):
    m = TILES[t][2]
    for k in (16, 32, 48, 64):
        xg, wf, wd, b, dyg, mg = problem(7 * k + t, H, W, k, m)
        pk3, dpk3 = ops.pack_x3(wf), ops.pack_x3(wd, dgrad=True)
        out["fwd", t, k] = ops.conv3x3_x3(xg, pk3, b, m, relu=True, tile=t).cpu()
        out["dgrad", t, k] = ops.conv3x3_x3(dyg, dpk3, None, m, mask=mg, tile=t).cpu()
        for grid in (5, 7):
            if grid > units(t, H, W, k, m):
                continue
            out["sk", t, k, grid] = ops.conv3x3_x3_streamk(xg, pk3, b, m, relu=True, tile=t, grid=grid).cpu()
            out["skdgrad", t, k, grid] = ops.conv3x3_x3_streamk(dyg, dpk3, None, m, mask=mg, tile=t, grid=grid).cpu()
        if k in (48, 64):
            out["splitk", t, k] = ops.conv3x3_splitk(xg, ops.pack_fwd(wf), b, m, 3, relu=True, tile=200 + t, dtype=F32_X3).cpu()
            out["splitkdgrad", t, k] = ops.conv3x3_splitk(dyg, ops.pack_dgrad(wd), None, m, 3, mask=mg, tile=200 + t, dtype=F32_X3).cpu()
        if k == 48:
            out["stride", t] = ops.conv3x3_x3(xg, pk3, b, m, relu=False, y_cs=m + 8, tile=t).cpu()
    for k in (32, 48, 64):                 # the fused pool forward on an even frame
        xg, wf, wd, b, dyg, mg = problem(11 * k + t, 16, 64, k, m)
        pk3 = ops.pack_x3(wf)
        for grid in (5, 7):
            if grid > units(t, 16, 64, k, m):
                continue
            y, p = ops.conv3x3_x3_streamk(xg, pk3, b, m, relu=True, tile=t, grid=grid, want_pooled=True)
            out["skpool.y", t, k, grid] = y.cpu()
            out["skpool.p", t, k, grid] = p.cpu()
torch.cuda.synchronize()
torch.save(out, sys.argv[2])
"""


def _run(pipe, tmp_path):
    path = str(tmp_path / ("early_pipe%d.pt" % pipe))
    env = dict(os.environ, OSVOS_X3_PIPE=str(pipe))
    r = subprocess.run([sys.executable, "-c", CHILD, REPO, path], env=env, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (pipe, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return torch.load(path)


def test_x3_early_barrier_is_bit_identical(tmp_path):
    old = _run(0, tmp_path)
    new = _run(1, tmp_path)
    assert old.keys() == new.keys()
    # every family of cases is present, stream-K with both grids and with one-chunk segments included
    for fam in ("fwd", "dgrad", "sk", "skdgrad", "splitk", "splitkdgrad", "stride", "skpool.y", "skpool.p"):
        assert any(key[0] == fam for key in new), fam
    assert ("sk", 10, 32, 7) in new and ("skdgrad", 14, 64, 5) in new and ("skpool.p", 12, 32, 7) in new
    bad = [key for key in old if not torch.equal(old[key], new[key])]
    assert not bad, bad[:10]
    assert all(torch.isfinite(v).all() for v in new.values())
    assert all(v.abs().max() > 0 for v in new.values())
