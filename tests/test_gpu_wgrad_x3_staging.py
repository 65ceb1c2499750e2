"""The branch-free staging addresses of wgrad_f32x3_kernel (csrc/wgrad_f32x3.hip): each staged item's patch-invariant byte offset and column
are computed once per thread, a stage adds the patch origin and does one unsigned column compare and a select.  The address form it replaces
is kept for one A/B behind OSVOS_WGRAD_X3_OLDADDR=1 (three- and two-piece bf16 forms; the FP16-pair "h2" forms have the new one only).

Shapes (N, H, W, Cin, Cout), chosen so that every address guard is the one that matters; plans as ops.wgrad_wide_plan reports them:

    3,6,5,64,64      ph 6, W below the patch width, 3 one-patch images walked by ONE workgroup (per_split 3, 1 split)
    2,7,19,64,64     ph 4, 2 x 2 patches per image: a right patch with 3 live columns, a bottom patch with 3 live rows, per_split 2
                     (under today's split rule no split of this shape holds patches of two images: 4 patches per image, 2 per split;
                      the walk from one image into the next is the first shape's)
    2,12,21,64,128   ph 6, two cout tiles, right patches with 5 live columns, per_split 2
    1,13,33,128,64   ph 4, a third patch column with ONE live column, a bottom patch with one live row, two cin tiles, per_split 2
    2,7,19,128,16    S16 (128 cins x 16 couts), ph 4, per_split 2
    1,12,37,256,16   S16, three patch columns, two cin tiles, per_split 3

a. bit identity: random fp32 operands, both address forms, overwrite and accumulate mode, precisions fp32x3 and fp32x2: dw and db byte-equal.
b. exactness with poisoned surroundings: small-integer operands (every partial sum exact in fp32; the float64 references stay below 126,
   far under 2^24), x and dy contiguous views from the middle of NaN-filled allocations with two image rows of NaN on either side, results
   written into NaN-filled dw / db: the result EQUALS the float64 gradient.  Run in both arms, and for the h2 kinds too (new form in both).

The switch is read once per process, so each arm runs in a child process of its own; one pair of children covers every case."""
import os
import subprocess
import sys

import pytest
import torch

import wide_wgrad_cases as wc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = [(3, 6, 5, 64, 64), (2, 7, 19, 64, 64), (2, 12, 21, 64, 128), (1, 13, 33, 128, 64)]
S16 = [(2, 7, 19, 128, 16), (1, 12, 37, 256, 16)]
SHAPES = WIDE + S16
# (ph, patches per image in x, in y, per_split > 1, cout tiles, cin tiles) each case relies on
FACTS = {(3, 6, 5, 64, 64): (6, 1, 1, 3, 1, 1), (2, 7, 19, 64, 64): (4, 2, 2, 2, 1, 1), (2, 12, 21, 64, 128): (6, 2, 2, 2, 2, 1),
         (1, 13, 33, 128, 64): (4, 3, 4, 2, 1, 2), (2, 7, 19, 128, 16): (4, 2, 2, 2, 1, 1), (1, 12, 37, 256, 16): (4, 3, 3, 3, 1, 2)}
BIT_KINDS = {False: ["x3", "x3b2"], True: ["x3_s16", "x3b2_s16"]}               # precisions fp32x3 and fp32x2
EXACT_KINDS = {False: ["x3", "x3b2", "x3h2"], True: ["x3_s16", "x3b2_s16", "x3h2_s16"]}

CHILD = r"""
import ctypes as C, os, sys, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import wide_wgrad_cases as wc
import test_gpu_wgrad_x3_staging as me
from osvos_pytorch_amd import _lib, ops
from osvos_pytorch_amd._lib import F32_X3
NAN = float("nan")
def poisoned(t):
    # a contiguous view of t's values from the middle of a NaN-filled allocation, two image rows (and 16-byte multiples) of NaN on either side
    n, h, w, c = t.shape
    pad = (2 * w * c + 3) // 4 * 4
    buf = torch.full((pad + t.numel() + pad,), NAN, device="cuda")
    buf[pad:pad + t.numel()] = t.reshape(-1).cuda()
    return buf[pad:pad + t.numel()].view(n, h, w, c), buf
def into(xg, dyg, cin, cout, dw, db):
    l = _lib.lib()
    n, h, w, cin_s = xg.shape
    p = lambda t: C.c_void_p(t.data_ptr())
    ws = torch.empty(l.osvos_wgrad_ws_bytes(n, h, w, cin_s, cout, F32_X3), device="cuda", dtype=torch.uint8)
    _lib.check(l.osvos_conv3x3_wgrad(p(xg), p(dyg), p(ws), p(dw), p(db), n, h, w, cin, cin_s, cout, dyg.shape[3], 0, F32_X3,
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)), "wgrad")
out = {}
for shape in me.SHAPES:
    cin, cout = shape[3], shape[4]
    x, dy = wc.random_operands(shape)
    xg, dyg = wc.x_nhwc(x).cuda(), wc.dy_nhwc(dy).cuda()
    g = torch.Generator().manual_seed(17 + cin + cout)
    dw0, db0 = torch.randn(cout, cin, 3, 3, generator=g).cuda(), torch.randn(cout, generator=g).cuda()
    xi, dyi = wc.integer_operands(shape)
    (xp, keep_x), (dyp, keep_dy) = poisoned(wc.x_nhwc(xi)), poisoned(wc.dy_nhwc(dyi))
    for kind in me.BIT_KINDS[cout == 16]:
        ops.set_x3_pieces(wc.KINDS[kind][2])
        dw, db = ops.conv3x3_wgrad(xg, dyg, cin, cout, dtype=F32_X3)
        out["over", shape, kind] = (dw.cpu(), db.cpu())
        dw, db = ops.conv3x3_wgrad(xg, dyg, cin, cout, dtype=F32_X3, accumulate_into=(dw0.clone(), db0.clone()))
        out["acc", shape, kind] = (dw.cpu(), db.cpu())
    for kind in me.EXACT_KINDS[cout == 16]:
        ops.set_x3_pieces(wc.KINDS[kind][2])
        dw, db = torch.full((cout, cin, 3, 3), NAN, device="cuda"), torch.full((cout,), NAN, device="cuda")
        into(xp, dyp, cin, cout, dw, db)
        out["exact", shape, kind] = (dw.cpu(), db.cpu())
    ops.set_x3_pieces(3)
torch.cuda.synchronize()
torch.save(out, sys.argv[2])
"""


def _run(oldaddr, tmp):
    path = str(tmp / ("staging_oldaddr%d.pt" % oldaddr))
    env = dict(os.environ, OSVOS_WGRAD_X3_OLDADDR=str(oldaddr))
    r = subprocess.run([sys.executable, "-c", CHILD, REPO, path], env=env, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (oldaddr, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return torch.load(path)


@pytest.fixture(scope="module")
def arms(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("wgrad_x3_staging")
    new = _run(0, tmp)
    old = _run(1, tmp)
    return new, old


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_plan_facts_the_cases_rely_on(shape):
    """the regime each shape is here for, through the library's own plan query, so a rule change cannot silently empty a case"""
    p = wc.plan(shape, "x3_s16" if shape[4] == 16 else "x3")
    ph, npx, npy, per_split, nco_t, nci_t = FACTS[shape]
    n, h, w = shape[:3]
    assert (p["pw"], p["ph"], p["npx"], p["npy"], p["nco_t"], p["nci_t"]) == (16, ph, npx, npy, nco_t, nci_t)
    assert p["npatches"] == n * npx * npy
    assert p["per_split"] == per_split and per_split > 1                 # every workgroup prefetches a live next patch and a dead one
    if shape == (3, 6, 5, 64, 64):
        assert p["nsplit"] == 1 and w < p["pw"] and wc.spanning_splits(p) == [0]      # one workgroup walks the three images
    if shape == (2, 7, 19, 64, 64):
        assert w - 16 * (npx - 1) == 3 and h - ph * (npy - 1) == 3
    if shape == (1, 13, 33, 128, 64):
        assert w - 16 * (npx - 1) == 1 and h - ph * (npy - 1) == 1


@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_address_forms_are_bit_identical(arms, shape):
    """a. random fp32 operands; the new and the old address form, overwrite and accumulate mode, fp32x3 and fp32x2: byte-equal dw and db"""
    new, old = arms
    for kind in BIT_KINDS[shape[4] == 16]:
        for mode in ("over", "acc"):
            (dw_n, db_n), (dw_o, db_o) = new[mode, shape, kind], old[mode, shape, kind]
            assert torch.isfinite(dw_n).all() and torch.isfinite(db_n).all() and dw_n.abs().max() > 0 and db_n.abs().max() > 0
            assert torch.equal(dw_n.view(torch.int32), dw_o.view(torch.int32)), (mode, kind, int((dw_n != dw_o).sum()))
            assert torch.equal(db_n.view(torch.int32), db_o.view(torch.int32)), (mode, kind, int((db_n != db_o).sum()))
        assert not torch.equal(new["over", shape, kind][0], new["acc", shape, kind][0])


@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_exact_gradient_with_poisoned_surroundings(arms, shape):
    """b. integer operands as views from the middle of NaN-filled allocations, results into NaN-filled buffers: EQUAL to float64"""
    _, _, dw_ref, db_ref = wc.integer_case(shape)
    assert dw_ref.abs().max() < 2 ** 24 and db_ref.abs().max() < 2 ** 24
    for arm, res in zip(("new", "old"), arms):
        for kind in EXACT_KINDS[shape[4] == 16]:
            dw, db = res["exact", shape, kind]
            assert torch.equal(dw.double(), dw_ref), (arm, kind, int((dw.double() != dw_ref).sum()), dw_ref.numel())
            assert torch.equal(db.double(), db_ref), (arm, kind, int((db.double() != db_ref).sum()), db_ref.numel())
