"""Masked data gradients, ReLU epilogues and the pooling kernels on REAL post-ReLU operands (tests/relu_mask_cases.py): about half of the mask
exactly +0.0, planted -0.0, 2^-126 and 2^-100, whole 32-channel blocks dead or live, a dead image row.  The rule is y = 0 where mask <= 0
(csrc/kernels.h, csrc/maskbits.h); the reference is float64 conv2d_input(...) * (mask > 0) -- autograd of vgg_osvos.py's conv -> ReLU -> conv,
tied to it in test_relu_mask_cases_cpu.py.  Every masked entry point is held, with relu=False, to
  (a) an exact zero wherever mask <= 0,
  (b) the bits of the same call without a mask (same tile, split, grid) wherever mask > 0,
  (c) the float64 bar the existing test of that entry point uses (3e-5 of the largest reference value for an fp32 result; for the bf16-only
      result of conv3x3_bf16act_fused its own |err| <= 2^-8 |ref| + 1e-3), the bf16 family against the reference on the bf16-rounded operands,
  (d) conv3x3_bf16io: bf16 mask == fp32 mask holding the same values, bit for bit,
  (e) conv3x3_bf16act_fused: one-bit mask == conv3x3_bf16io's bf16 result under the tensor mask on the same tile, bit for bit.
(a) and (b) need no tolerance: a kernel that tests the sign bit, uses >= 0, reads a bf16 mask as an unsigned pattern, leaves stale memory in a
dead block or treats the split-K finalize differently fails them.  Stale memory: every masked call writes into a result buffer filled with NaN
beforehand (`out=` of the ops wrappers), as the network writes into reused workspace -- a store skipped for a dead element, one-bit word or
block leaves a NaN there and fails (a), whatever the allocator would have handed out."""
import functools

import pytest
import torch
import torch.nn.functional as F

import relu_mask_cases as rc

pytestmark = pytest.mark.gpu

F32_BAR = 3e-5          # test_conv3x3_dgrad_and_wgrad, test_conv3x3_f32x3_streamk, test_conv3x3_bf16_mfma_rounding_and_dgrad: max error / max |ref|


def _ops():
    from osvos_pytorch_amd import ops
    return ops


def nhwc(t):  # cpu NCHW -> cuda NHWC contiguous, dtype kept
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(t):  # cuda NHWC -> cpu NCHW float64
    return t.permute(0, 3, 1, 2).double().cpu()


def max_err(a, ref):
    return float((a.double() - ref).abs().max() / (ref.abs().max() + 1e-30))


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def poison(c, dtype=torch.float32):
    """the result buffer of a masked call: NaN everywhere, so that an element the kernel does not store cannot read back as a zero"""
    return torch.full(tuple(c.live.shape), float("nan"), device="cuda", dtype=dtype)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(layer):
    """operands and float64 references of one layer's data gradient, built once (CPU references stay untouched)"""
    n, h, w, cin, cout = layer
    c = Case()
    g = torch.Generator().manual_seed(rc.layer_seed(layer))
    c.x_shape = (n, cin, h, w)
    c.wt = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cout ** 0.5)
    c.dy = torch.randn(n, cout, h, w, generator=g)
    c.m = rc.post_relu_mask(c.x_shape, rc.layer_seed(layer), torch.float32)
    c.mb = rc.post_relu_mask(c.x_shape, rc.layer_seed(layer), torch.bfloat16)
    assert torch.equal(c.m > 0, c.mb > 0)
    c.ref = rc.expected_dx(c.x_shape, c.wt, c.dy, c.m)
    c.ref16 = rc.expected_dx(c.x_shape, c.wt.bfloat16(), c.dy.bfloat16(), c.mb)
    c.dyg, c.mg, c.mbg = nhwc(c.dy), nhwc(c.m), nhwc(c.mb)
    c.live = c.mg > 0
    c.dead = ~c.live
    assert torch.equal(c.dead, c.mbg <= 0) and 0.35 <= float(c.dead.float().mean()) <= 0.65
    return c


def check(tag, c, masked, plain, ref=None, bar=F32_BAR):
    """(a), (b) and, with a reference, (c).  Prints the figure before asserting."""
    assert masked.shape == c.live.shape and plain.shape == c.live.shape, tag
    assert not bool(torch.isnan(masked).any()), ("(a) elements never stored (the NaN of the pre-filled result buffer)", tag, int(torch.isnan(masked).sum()))
    assert bool((masked[c.dead] == 0).all()), ("(a) non-zero where mask <= 0", tag, int((masked[c.dead] != 0).sum()))
    assert torch.equal(bits(masked)[c.live], bits(plain)[c.live]), ("(b) differs from the unmasked call where mask > 0", tag)
    if ref is not None:
        e = max_err(nchw(masked), ref)
        print("%s: max err / max |ref| = %.2e" % (tag, e))
        assert e < bar, ("(c)", tag, e)


ALL_LAYERS = rc.LAYERS + [rc.DEEP]


@pytest.mark.parametrize("tile", [-1, 9, 109])
@pytest.mark.parametrize("layer", rc.LAYERS, ids=str)
def test_exact_fp32_tensor_mask(layer, tile):
    ops = _ops()
    c = case(layer)
    cin = layer[3]
    dpk = ops.pack_dgrad(c.wt.cuda())
    dx = ops.conv3x3(c.dyg, dpk, None, cin, mask=c.mg, tile=tile, out=poison(c))
    check(("conv3x3", layer, tile), c, dx, ops.conv3x3(c.dyg, dpk, None, cin, tile=tile), c.ref)


@pytest.mark.parametrize("tile", [205, 210, 212, 214])
@pytest.mark.parametrize("layer", rc.LAYERS, ids=str)
def test_f32x3_tensor_mask(layer, tile):
    from osvos_pytorch_amd._lib import F32_X3
    ops = _ops()
    c = case(layer)
    cin = layer[3]
    dpk = ops.pack_dgrad(c.wt.cuda())
    dx = ops.conv3x3(c.dyg, dpk, None, cin, mask=c.mg, tile=tile, dtype=F32_X3, out=poison(c))
    check(("conv3x3 F32_X3", layer, tile), c, dx, ops.conv3x3(c.dyg, dpk, None, cin, tile=tile, dtype=F32_X3), c.ref)


@pytest.mark.parametrize("tile", [-1, 10, 12, 14, 16])
@pytest.mark.parametrize("layer", rc.LAYERS, ids=str)
def test_f32x3_presplit_tensor_mask(layer, tile):
    ops = _ops()
    c = case(layer)
    cin = layer[3]
    dpk3 = ops.pack_x3(c.wt.cuda(), dgrad=True)
    dx = ops.conv3x3_x3(c.dyg, dpk3, None, cin, mask=c.mg, tile=tile, out=poison(c))
    check(("conv3x3_x3", layer, tile), c, dx, ops.conv3x3_x3(c.dyg, dpk3, None, cin, tile=tile), c.ref)


@pytest.mark.parametrize("ksplit", [2, 3, 8])
@pytest.mark.parametrize("arith", ["exact", "f32x3"])
@pytest.mark.parametrize("layer", ALL_LAYERS, ids=str)
def test_splitk_finalize_tensor_mask(layer, arith, ksplit):
    """The finalize kernel's mask.  The launchers cut K only while ksplit <= kernel Cin / 8 (exact) or / 16 (f32x3), where the kernel's Cin is the
    layer's Cout (64, 128, 64 and DEEP's 256).  So the finalize kernel runs in every exact case (ksplit 2, 3, 8 on all four layers) and in the
    f32x3 cases with ksplit 2 and 3 on all four layers and ksplit 8 on (1, 33, 70, 64, 128) and DEEP.  The two left over, f32x3 with ksplit 8
    on the layers whose Cout is 64, run un-split through the plain epilogue and are held to the same checks.  If the caps change, keep at
    least ksplit 2 and 3 of either arithmetic on DEEP in this list: they are what the test is for."""
    from osvos_pytorch_amd._lib import F32, F32_X3
    ops = _ops()
    c = case(layer)
    cin = layer[3]
    dpk = ops.pack_dgrad(c.wt.cuda())
    tile, dtype = (-1, F32) if arith == "exact" else (205, F32_X3)
    dx = ops.conv3x3_splitk(c.dyg, dpk, None, cin, ksplit, mask=c.mg, tile=tile, dtype=dtype, out=poison(c))
    plain = ops.conv3x3_splitk(c.dyg, dpk, None, cin, ksplit, tile=tile, dtype=dtype)
    check(("conv3x3_splitk", layer, arith, ksplit), c, dx, plain, c.ref)


@pytest.mark.parametrize("grid", [0, 5, 7])
@pytest.mark.parametrize("tile", [12, 14])
@pytest.mark.parametrize("layer", ALL_LAYERS, ids=str)
def test_streamk_tensor_mask(layer, tile, grid):
    """Grids 5 and 7 force stream-K on every layer here (the launcher asks for at least as many work units, tiles x kernel Cin / 16, as
    workgroups: the smallest layer has 16).  Grid 0 leaves the choice to the launcher, which at these sizes has fewer units than the chip has
    CUs and takes the plain grid: that launch goes through the same entry point and is held to the same checks, but it is the forced grids
    that reach the stream-K fix-up epilogue."""
    ops = _ops()
    c = case(layer)
    cin = layer[3]
    dpk3 = ops.pack_x3(c.wt.cuda(), dgrad=True)
    dx = ops.conv3x3_x3_streamk(c.dyg, dpk3, None, cin, mask=c.mg, tile=tile, grid=grid, out=poison(c))
    plain = ops.conv3x3_x3_streamk(c.dyg, dpk3, None, cin, tile=tile, grid=grid)
    check(("conv3x3_x3_streamk", layer, tile, grid), c, dx, plain, c.ref)
    ws = ops.streamk_workspace(c.dyg.device)
    assert int(ws[:ops.lib().osvos_conv3x3_x3_streamk_ticket_bytes()].view(torch.int32).abs().max()) == 0


def bf16_tiles(ops, kcin, kcout):
    """the filter of test_conv3x3_bf16act_fused_epilogues_every_tile, on the channels the KERNEL sees (a data gradient maps Cout -> Cin)"""
    return [t for t in ops.conv3x3_bf16io_tiles() if (t < 36 or kcin == 64) and (t < 30 or (kcin % 16 == 0 and kcout % 8 == 0))]


@pytest.mark.parametrize("layer", rc.LAYERS, ids=str)
def test_bf16io_fp32_and_bf16_tensor_masks(layer):
    """conv3x3_bf16io (bf16 dy from HBM, fp32 + bf16 results) on every tile the shape admits: fp32 mask, bf16 mask, and (d) the two bit for bit"""
    from osvos_pytorch_amd._lib import F32_BF16MFMA
    ops = _ops()
    c = case(layer)
    n, h, w, cin, cout = layer
    dpk = ops.pack_dgrad(c.wt.cuda(), F32_BF16MFMA)
    dyb = c.dyg.bfloat16()
    tiles = bf16_tiles(ops, cout, cin)
    assert (36 in tiles) == (cout == 64) and 8 in tiles and 30 in tiles
    mb_as_f32 = c.mbg.float()
    bad = []
    for tile in tiles:
        p32, p16 = ops.conv3x3_bf16io(dyb, dpk, None, cin, tile=tile)
        for name, mask in (("fp32 mask", c.mg), ("bf16 mask", c.mbg)):
            y32, y16 = ops.conv3x3_bf16io(dyb, dpk, None, cin, mask=mask, tile=tile, out=(poison(c), poison(c, torch.bfloat16)))
            try:
                check(("conv3x3_bf16io", name, layer, tile), c, y32, p32, c.ref16)
                check(("conv3x3_bf16io bf16 result", name, layer, tile), c, y16, p16)
                assert torch.equal(bits(y16), bits(y32.bfloat16())), ("bf16 copy", name, layer, tile)
            except AssertionError as e:
                bad.append(str(e)[:300])
            if name == "bf16 mask":
                z32, z16 = ops.conv3x3_bf16io(dyb, dpk, None, cin, mask=mb_as_f32, tile=tile, out=(poison(c), poison(c, torch.bfloat16)))
                if not (torch.equal(bits(z32), bits(y32)) and torch.equal(bits(z16), bits(y16))):
                    bad.append("(d) bf16 mask != fp32 mask of the same values, tile %d" % tile)
    assert not bad, bad


@pytest.mark.parametrize("layer", rc.LAYERS, ids=str)
def test_bf16act_fused_one_bit_mask(layer):
    """conv3x3_bf16act_fused(mask_bits=...) on every tile the shape admits (and the Cin = 64 persistent kernel, tile 38): the words packed on the
    host from the same mask by maskbits.h's rule"""
    from osvos_pytorch_amd._lib import F32_BF16MFMA
    ops = _ops()
    c = case(layer)
    n, h, w, cin, cout = layer
    dpk = ops.pack_dgrad(c.wt.cuda(), F32_BF16MFMA)
    dyb = c.dyg.bfloat16()
    mbits = rc.pack_mask_bits(c.mbg.cpu()).cuda()
    io_tiles = bf16_tiles(ops, cout, cin)
    bad = []
    for tile in io_tiles + ([38] if cout == 64 else []):
        d, _, _, _ = ops.conv3x3_bf16act_fused(dyb, dpk, None, cin, relu=False, mask_bits=mbits, tile=tile, out=poison(c, torch.bfloat16))
        plain, _, _, _ = ops.conv3x3_bf16act_fused(dyb, dpk, None, cin, relu=False, tile=tile)
        try:
            check(("conv3x3_bf16act_fused", layer, tile), c, d, plain)
            err = (nchw(d.float()) - c.ref16).abs()
            worst = float((err / (c.ref16.abs() * 2.0 ** -8 + 1e-3)).max())
            print("conv3x3_bf16act_fused %s tile %d: worst err / (2^-8 |ref| + 1e-3) = %.3f" % (layer, tile, worst))
            assert worst <= 1.0, ("(c)", layer, tile, worst)
            if tile in io_tiles:
                _, y16 = ops.conv3x3_bf16io(dyb, dpk, None, cin, mask=c.mbg, tile=tile, want_f32=False, out=(None, poison(c, torch.bfloat16)))
                assert torch.equal(bits(d), bits(y16)), ("(e) one-bit mask != tensor mask", layer, tile)
        except AssertionError as e:
            bad.append(str(e)[:300])
    assert not bad, bad


# ---- forward side: a ReLU epilogue on an exactly-zero pre-activation

BIAS_CYCLE = (0.0, -0.0, rc.TINY, -rc.TINY, 1.0, -1.0)


def _zero_preactivation(layer):
    n, h, w, cin, cout = layer
    g = torch.Generator().manual_seed(rc.layer_seed(layer) + 1)
    x = nhwc(torch.randn(n, cin, h, w, generator=g))
    wt = torch.zeros(cout, cin, 3, 3).cuda()
    b = torch.tensor([BIAS_CYCLE[k % 6] for k in range(cout)])
    assert bool(torch.signbit(b[1])) and not bool(torch.signbit(b[0]))
    want = torch.clamp(b, min=0).cuda().expand(n, h, w, cout)              # max(bias, 0) per channel: both zeros and both negatives give zero
    return x, wt, b.cuda(), want


def _is(y, want):
    return y.shape == want.shape and bool((y.float() == want).all())


@pytest.mark.parametrize("layer", rc.LAYERS, ids=str)
def test_relu_epilogue_on_zero_preactivation_fp32_families(layer):
    from osvos_pytorch_amd._lib import F32_X3
    ops = _ops()
    n, h, w, cin, cout = layer
    x, wt, b, want = _zero_preactivation(layer)
    pk, pk3 = ops.pack_fwd(wt), ops.pack_x3(wt)
    assert _is(ops.conv3x3(x, pk, b, cout, relu=True, tile=9), want)
    assert _is(ops.conv3x3(x, pk, b, cout, relu=True, tile=212, dtype=F32_X3), want)
    assert _is(ops.conv3x3_x3(x, pk3, b, cout, relu=True, tile=12), want)
    assert _is(ops.conv3x3_splitk(x, pk, b, cout, 2, relu=True, tile=9), want)                       # ReLU in the finalize kernel
    assert _is(ops.conv3x3_splitk(x, pk, b, cout, 2, relu=True, tile=205, dtype=F32_X3), want)
    y, pooled = ops.conv3x3_x3_streamk(x, pk3, b, cout, relu=True, tile=12, grid=5, want_pooled=True)
    assert _is(y, want)
    assert torch.equal(pooled, ops.maxpool2x2(y)) and _is(pooled, want[:, : (h + 1) // 2, : (w + 1) // 2])


@pytest.mark.parametrize("layer", rc.LAYERS, ids=str)
def test_relu_epilogue_on_zero_preactivation_bf16_family(layer):
    from osvos_pytorch_amd._lib import F32_BF16MFMA
    ops = _ops()
    n, h, w, cin, cout = layer
    x, wt, b, want = _zero_preactivation(layer)
    xb = x.bfloat16()
    pk = ops.pack_fwd(wt, F32_BF16MFMA)
    y32, y16 = ops.conv3x3_bf16io(xb, pk, b, cout, relu=True, tile=8)
    assert _is(y32, want) and _is(y16, want)
    positive = [k for k in range(cout) if BIAS_CYCLE[k % 6] > 0]
    want_words = torch.tensor([sum(1 << (k - 32 * g) for k in positive if 32 * g <= k < 32 * g + 32) for g in range(cout // 32)])
    dy = nhwc(torch.randn(n, cout, (h + 1) // 2, (w + 1) // 2, generator=torch.Generator().manual_seed(3))).bfloat16()
    for tile in [8, 30] + ([36, 38] if cin == 64 else []):
        y, ybits, _, _ = ops.conv3x3_bf16act_fused(xb, pk, b, cout, relu=True, want_bits=True, tile=tile)
        assert _is(y, want), tile
        assert bool(((ybits.cpu().long() & 0xFFFFFFFF) == want_words).all()), tile            # a bit only for the two positive biases
        y1, _, pooled, code = ops.conv3x3_bf16act_fused(xb, pk, b, cout, relu=True, want_pool=True, tile=tile)
        assert torch.equal(bits(y1), bits(y)), tile
        assert torch.equal(bits(pooled), bits(ops.maxpool2x2_bf16act(y))), tile
        assert _is(pooled, want[:, : (h + 1) // 2, : (w + 1) // 2]), tile
        for side in (None, torch.ones_like(y)):
            a = ops.maxpool2x2_bwd_bf16act_code(code, dy, (h, w), side)
            assert torch.equal(bits(a), bits(ops.maxpool2x2_bwd_bf16act(y, dy, side))), (tile, side is None)
            assert bool((a[want == 0] == 0).all()), tile                                      # nothing flows into a channel whose output is zero


# ---- pooling on post-ReLU zeros

@functools.lru_cache(maxsize=None)
def pool_case(shape, bf16):
    """input, upstream and side gradients (bf16-representable for the bf16 kernels) and the float64 references, built once per shape"""
    n, ch, h, w = shape
    c = Case()
    seed = 7 + ch + 100 * h + w
    c.x = rc.pool_input(shape, seed, torch.bfloat16 if bf16 else torch.float32).float()
    g = torch.Generator().manual_seed(seed)
    xd = c.x.double().requires_grad_()
    c.y = F.max_pool2d(xd, 2, 2, ceil_mode=True)
    c.dy = torch.randn(c.y.shape, generator=g)
    c.side = torch.randn(shape, generator=g)
    if bf16:
        c.dy, c.side = c.dy.bfloat16().float(), c.side.bfloat16().float()
    c.y.backward(c.dy.double())
    c.y = c.y.detach()
    live = c.x > 0
    c.ref_side = (xd.grad + c.side.double()) * live
    c.ref_plain = xd.grad * live
    c.zero_windows = nhwc(rc.all_zero_windows(c.x))
    assert int(c.zero_windows.sum()) > 0
    return c


def _pool_backward_checks(tag, c, dx_side, dx_plain, round_to_bf16):
    ref_side, ref_plain = c.ref_side, c.ref_plain
    if round_to_bf16:      # the kernel adds in fp32 and rounds once (RNE): the float64 sum of two bf16 values, rounded to fp32, then to bf16
        ref_side, ref_plain = ref_side.float().bfloat16().double(), ref_plain.float().bfloat16().double()
    for name, dx, ref in (("side", dx_side, ref_side), ("plain", dx_plain, ref_plain)):
        e = max_err(nchw(dx), ref)
        print("%s %s: max err / max |ref| = %.2e" % (tag, name, e))
        assert e < 1e-6, (tag, name, e)
        assert bool((dx[c.zero_windows] == 0).all()), (tag, name, "gradient inside an all-zero window")


@pytest.mark.parametrize("hw", rc.POOL_HW, ids=str)
@pytest.mark.parametrize("ch", rc.POOL_C)
def test_maxpool_fp32_and_bf16copy_on_post_relu_zeros(ch, hw):
    ops = _ops()
    c = pool_case((rc.POOL_N, ch) + hw, False)
    xg, dyg, sg = nhwc(c.x), nhwc(c.dy), nhwc(c.side)
    y = ops.maxpool2x2(xg)
    assert torch.equal(nchw(y), c.y)
    _pool_backward_checks(("maxpool2x2_bwd", ch, hw), c, ops.maxpool2x2_bwd(xg, dyg, sg), ops.maxpool2x2_bwd(xg, dyg, None), False)
    y2, y2b = ops.maxpool2x2_bf16copy(xg)
    assert torch.equal(nchw(y2), c.y) and torch.equal(bits(y2b), bits(y2.bfloat16()))
    d1, d1b = ops.maxpool2x2_bwd_bf16copy(xg, dyg, sg)
    d0, d0b = ops.maxpool2x2_bwd_bf16copy(xg, dyg, None)
    _pool_backward_checks(("maxpool2x2_bwd_bf16copy", ch, hw), c, d1, d0, False)
    assert torch.equal(bits(d1b), bits(d1.bfloat16())) and torch.equal(bits(d0b), bits(d0.bfloat16()))
    assert bool((d1b[c.zero_windows] == 0).all()) and bool((d0b[c.zero_windows] == 0).all())


@pytest.mark.parametrize("hw", rc.POOL_HW, ids=str)
@pytest.mark.parametrize("ch", rc.POOL_C)
def test_maxpool_bf16act_on_post_relu_zeros(ch, hw):
    ops = _ops()
    c = pool_case((rc.POOL_N, ch) + hw, True)
    xg, dyg, sg = nhwc(c.x).bfloat16(), nhwc(c.dy).bfloat16(), nhwc(c.side).bfloat16()
    assert torch.equal(xg.float(), nhwc(c.x)) and torch.equal(dyg.float(), nhwc(c.dy))          # bf16-representable: nothing is rounded here
    y = ops.maxpool2x2_bf16act(xg)
    assert torch.equal(nchw(y), c.y)
    yc, code = ops.maxpool2x2_bf16act_code(xg)
    assert torch.equal(nchw(yc), c.y)
    _pool_backward_checks(("maxpool2x2_bwd_bf16act", ch, hw), c, ops.maxpool2x2_bwd_bf16act(xg, dyg, sg), ops.maxpool2x2_bwd_bf16act(xg, dyg, None), True)
    _pool_backward_checks(("maxpool2x2_bwd_bf16act_code", ch, hw), c, ops.maxpool2x2_bwd_bf16act_code(code, dyg, hw, sg),
                          ops.maxpool2x2_bwd_bf16act_code(code, dyg, hw, None), True)
