"""Pins tests/wide_wgrad_cases.py, the shapes and operands of test_gpu_wide_wgrad.py: through the library's own plan query
(osvos_wgrad_wide_plan, host only: the launchers' make_plan3 / make_plan and their form and block-map selection) every regime the GPU tests
claim to reach is asserted here, per kernel family, so a later retune of the split targets fails loudly instead of silently returning the
tests to short walks.  Also the conditions the exact-equality tests rest on: operands that are exact in bf16, in FP16 at the block scale
and in fp32, partial sums below 2^24, integral non-zero references -- and the workspace arithmetic."""
import pytest
import torch

import wide_wgrad_cases as wc


def _ids(pairs):
    return ["%s-%s" % ("x".join(map(str, s)), k) for s, k in pairs]


@pytest.mark.parametrize("shape,kind", list(wc.TABLE), ids=_ids(list(wc.TABLE)))
def test_plan_is_the_table(shape, kind):
    n, h, w, cin, cout = shape
    p = wc.plan(shape, kind)
    assert (p["pw"], p["ph"]) == ((16, p["ph"]) if kind.startswith("x3") else (32, 8)) and p["ph"] in (4, 6, 8)
    assert p["npx"] == -(-w // p["pw"]) and p["npy"] == -(-h // p["ph"]) and p["npatches"] == n * p["npx"] * p["npy"]
    assert p["nsplit"] == -(-p["npatches"] // p["per_split"]) and (p["nsplit"] - 1) * p["per_split"] < p["npatches"]
    bco = 32 if kind.endswith("_s16") else (128 if p["wide"] else 64)
    assert p["nco_t"] == -(-cout // bco) and p["nci_t"] == -(-cin // (128 if kind.endswith("_s16") else 64))
    assert p["blocks"] == p["nsplit"] * p["nco_t"] * p["nci_t"] and p["map"] == int(p["blocks"] % 8 == 0)
    assert p["wide"] == int(kind in ("bf16_act", "bf16_act16") and cout % 128 == 0)
    assert wc.table_row(p) == wc.TABLE[(shape, kind)], (shape, kind, wc.table_row(p))


def test_every_long_walk_case_has_its_row_and_the_pieces_do_not_change_the_plan():
    for shape, kind in wc.LONG:
        base = {"x3b2": "x3", "x3h2": "x3", "x3b2_s16": "x3_s16", "x3h2_s16": "x3_s16"}.get(kind, kind)
        assert (shape, base) in wc.TABLE, (shape, kind)
        assert wc.plan(shape, kind) == wc.plan(shape, base)
        assert kind in wc.kinds_for(shape)
    for shape, kind in wc.SCALED + wc.TINY:
        assert kind in wc.kinds_for(shape), (shape, kind)
        assert wc.plan(shape, kind)["npatches"] >= 1


FAMILIES = {
    "x3": [wc.plan(s, k) for (s, k) in wc.TABLE if k.startswith("x3")],
    "bf16": [wc.plan(s, k) for (s, k) in wc.TABLE if k.startswith("bf16")],
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_shapes_reach_every_regime_of_each_family(family):
    plans = FAMILIES[family]
    assert any(p["per_split"] >= 4 for p in plans)                                       # a prefetch issued under a prefetched patch, twice over
    assert any(p["per_split"] >= 4 and wc.tail(p) < p["per_split"] for p in plans)       # ... with a short last split
    assert any(p["per_split"] >= 4 and wc.spanning_splits(p) for p in plans)             # ... and a split with patches of two images
    assert {p["map"] for p in plans} == {0, 1}                                           # both arms of the block map
    assert any(p["nco_t"] > 1 and p["nci_t"] > 1 for p in plans)
    assert any(p["nsplit"] > 64 for p in plans)                                          # the shared reduce's `sp += 64` loop
    assert all(p["nsplit"] * p["per_split"] >= p["npatches"] for p in plans)
    if family == "x3":
        assert {p["ph"] for p in plans} == {4, 6}                                        # both patch heights
        assert any(p["nco_t"] > 1 and p["nci_t"] > 1 and p["map"] == 0 for p in plans)   # several tiles of both kinds in the plain order too
    else:
        assert {p["wide"] for p in plans} == {0, 1}                                      # the four-wave and the eight-wave form


def test_every_kernel_walks_a_short_tail_and_a_spanning_split():
    """beyond the per-family list: each kernel of its own -- the S16 form, wgrad_bf16_kernel<0>, wgrad_bf16pm_kernel<4> and <8>"""
    for kind, wide in (("x3", 0), ("x3_s16", 0), ("bf16_f32t", 0), ("bf16_act", 0), ("bf16_act", 1)):
        plans = [wc.plan(s, k) for (s, k) in wc.TABLE if k == kind]
        plans = [p for p in plans if p["wide"] == wide]
        assert any(p["per_split"] >= 3 and wc.tail(p) < p["per_split"] and wc.spanning_splits(p) for p in plans), (kind, wide)


@pytest.mark.parametrize("shape,kind", list(wc.TABLE), ids=_ids(list(wc.TABLE)))
def test_partial_last_patch_column_and_row(shape, kind):
    p = wc.plan(shape, kind)
    n, h, w = shape[:3]
    if shape in (wc.X3_LONG[0], wc.X3_LONG[2]):            # the two ph = 6 shapes: rows fill their patches, the last column does not
        assert w % p["pw"] != 0 and h % p["ph"] == 0
    else:
        assert w % p["pw"] != 0 and h % p["ph"] != 0


def test_the_tiny_shapes_are_one_workgroup_walking_every_patch():
    for shape, kind in wc.TINY:
        p = wc.plan(shape, kind)
        assert p["nsplit"] == 1 and p["blocks"] == 1 and p["per_split"] == p["npatches"] == shape[0], (shape, kind, p)
    # H below the patch height and W below the patch width, in both families
    assert wc.TINY_PIXELS[1][1] < 4 and wc.TINY_PIXELS[1][2] < 16


@pytest.mark.parametrize("shape", wc.OLD_X3_SHAPES, ids=str)
def test_the_earlier_f32x3_shapes_walk_at_most_three_patches_with_full_tails(shape):
    """the gap: no op-level shape fed to the f32x3 weight gradient before walked more than three patches or had a short last split, and
    only the single-workgroup (3,6,16,64,64) had a split spanning two images"""
    p = wc.plan(shape, "x3_s16" if shape[4] == 16 else "x3")
    assert p["per_split"] <= 3 and wc.tail(p) == p["per_split"] and p["nsplit"] * p["per_split"] == p["npatches"]
    assert not wc.spanning_splits(p) or shape == (3, 6, 16, 64, 64)


@pytest.mark.parametrize("bf16_tensors", [False, True], ids=["f32t", "act"])
@pytest.mark.parametrize("shape", wc.OLD_BF16_SHAPES, ids=str)
def test_the_earlier_bf16_shapes_walk_at_most_three_patches_with_full_tails(shape, bf16_tensors):
    p = wc.plan(shape, "bf16_act" if bf16_tensors else "bf16_f32t")
    assert p["per_split"] <= 3 and wc.tail(p) == p["per_split"] and not wc.spanning_splits(p)


def test_plan_query_rejects_bad_arguments():
    import ctypes as C
    from osvos_pytorch_amd import _lib
    from osvos_pytorch_amd._lib import F32, F32_BF16MFMA, F32_X3
    l, out = _lib.lib(), (C.c_int * 12)()
    assert l.osvos_wgrad_wide_plan(2, 8, 8, 64, 64, F32_X3, 0, out) == 0
    assert l.osvos_wgrad_wide_plan(2, 8, 8, 64, 64, F32_X3, 0, None) < 0           # no result array
    assert l.osvos_wgrad_wide_plan(0, 8, 8, 64, 64, F32_X3, 0, out) < 0            # empty tensor
    assert l.osvos_wgrad_wide_plan(2, 8, 8, 64, 48, F32_X3, 0, out) < 0            # not a wide layer
    assert l.osvos_wgrad_wide_plan(2, 8, 8, 64, 16, F32_X3, 0, out) < 0            # S16 needs Cin % 128 == 0
    assert l.osvos_wgrad_wide_plan(2, 8, 8, 8, 64, F32_BF16MFMA, 0, out) < 0       # conv1_1 is the skinny kernels'
    assert l.osvos_wgrad_wide_plan(2, 8, 8, 64, 16, F32_BF16MFMA, 0, out) < 0      # Cout 16 on fp32 tensors: the skinny kernel
    assert l.osvos_wgrad_wide_plan(2, 8, 8, 64, 16, F32_BF16MFMA, 1, out) == 0     # ... on bf16 tensors: the 64-cout tile
    assert l.osvos_wgrad_wide_plan(2, 8, 8, 64, 64, F32, 0, out) < 0               # the exact fp32 kernel is not a wide kernel
    assert l.osvos_wgrad_wide_plan(2, 8, 8, 64, 64, F32_X3, 1, out) < 0            # bf16 tensors go with the bf16 dtype


ALL_CASES = sorted(set(wc.LONG + wc.SCALED + wc.TINY + [(s, k) for s, _ in wc.STRIDED for k in wc.X3_KINDS + wc.BF16_KINDS]))


def test_workspace_query_covers_every_kind_and_shape():
    """the public size query is at least the kernel's own nsplit slabs and bias partials, for the dtype the entry point asks with"""
    from osvos_pytorch_amd import _lib
    for shape, kind in ALL_CASES:
        dtype = _lib.F32_X3 if wc.KINDS[kind][0] == "x3" else _lib.F32_BF16MFMA
        n, h, w, cin, cout = shape
        own = wc.own_ws_bytes(shape, wc.plan(shape, kind))
        assert own == wc.plan(shape, kind)["nsplit"] * (9 * cout * cin + cout) * 4
        assert _lib.lib().osvos_wgrad_ws_bytes(n, h, w, cin, cout, dtype) >= own, (shape, kind)


def _assert_fp16_at_block_scale(t, what):
    """h2split.h scales an operand so that its block's largest magnitude lands in [2^14, 2^15); the block is a workgroup's tile so far, so its
    maximum lies between the value itself and the tensor's largest: both extremes must leave every value an FP16 number"""
    gmax = float(t.abs().max())
    if gmax == 0:
        return
    for block_max in (gmax, 1.0):
        s = 2.0 ** (14 - torch.tensor(block_max).log2().floor())
        v = t * s
        v = v[v.abs() < 2.0 ** 16]                 # (under a block maximum of 1 the larger values belong to other blocks)
        assert torch.equal(v.half().float(), v), what


INTEGER_SHAPES = sorted(set(s for s, _ in wc.LONG + wc.TINY) | set(s for s, _ in wc.STRIDED))


@pytest.mark.parametrize("shape", INTEGER_SHAPES, ids=str)
def test_integer_operands_make_every_summation_order_exact(shape):
    n, h, w, cin, cout = shape
    x, dy, dw, db = wc.integer_case(shape)
    assert x.shape == (n, cin, h, w) and dy.shape == (n, cout, h, w)
    assert torch.equal(x, x.round()) and float(x.abs().max()) <= 3 and set(dy.unique().tolist()) <= {-1.0, 0.0, 1.0}
    if n * h * w >= 100:
        assert float(x.min()) == -3 and float(x.max()) == 3 and 0.4 < float((x == 0).float().mean()) < 0.6       # 40 % masked + 1/7 drawn zeros
    assert torch.equal(x.bfloat16().float(), x) and torch.equal(dy.bfloat16().float(), dy)      # exact in bf16
    _assert_fp16_at_block_scale(x, "x"), _assert_fp16_at_block_scale(dy, "dy")                   # ... and in FP16 at the block scale
    assert 3 * n * h * w < 2 ** 24                                                              # bound of every partial sum
    for t in (dw, db):
        assert t.dtype == torch.float64 and torch.equal(t, t.round()) and float(t.abs().max()) < 2 ** 24
    assert dw.shape == (cout, cin, 3, 3) and db.shape == (cout,)
    if n * h * w >= 15:
        assert float(dw.abs().max()) > 0 and float(db.abs().max()) > 0
    # narrower tensors are the leading channels of the same draw
    assert torch.equal(wc.integer_operands((n, h, w, 64, 16))[0], x[:, :64]) and torch.equal(wc.integer_operands((n, h, w, 64, 16))[1], dy[:, :16])


@pytest.mark.parametrize("schedule", wc.SCHEDULES)
@pytest.mark.parametrize("shape", wc.SCALED_SHAPES, ids=str)
def test_scaled_operands_are_exact_and_follow_the_walk(shape, schedule):
    n, h, w, cin, cout = shape
    x0, dy0 = wc.integer_operands(shape)
    x, dy, dw, db = wc.scaled_case(shape, schedule)
    a, b, live = wc.schedule_exponents(shape, schedule)
    patch, j, per_split = wc.patch_index(shape)
    p = wc.plan(shape, "x3_s16" if cout == 16 else "x3")
    assert per_split == p["per_split"] >= 3 and int(patch.max()) == p["npatches"] - 1 and int(j.max()) == per_split - 1
    assert torch.equal(patch[0, :p["ph"], :16], torch.zeros(min(h, p["ph"]), 16, dtype=torch.long)) and int(patch[0, 0, 16]) == 1
    # exponents are constant over a patch and follow the position in the split's walk
    for t in (a, b, live):
        for q in (0, 1, per_split, p["npatches"] - 1):
            assert t[patch == q].unique().numel() == 1
    first, last = j == 0, j == per_split - 1
    if schedule.startswith("rise"):
        assert int(a[last].min()) > int(a[first].max()) or schedule == "rise_x"
        assert int(b[last].min()) > int(b[first].max()) or schedule == "rise_dy"
        assert (a + b)[j == 1].min() > (a + b)[first].max() and (a + b)[last].min() > (a + b)[j == per_split - 2].max()      # drops at several patches
    elif schedule == "fall":
        assert int(a[first].min()) > int(a[last].max()) and int(b[first].min()) > int(b[last].max())
    else:
        assert int(live[first].max()) == 0 and int(live[j == per_split // 2].max()) == 0 and int(live[last].min()) == 1
        assert float(x[0, :, :p["ph"], :16].abs().max()) == 0 and float(dy[0, :, :p["ph"], :16].abs().max()) == 0       # the very first patch is all zeros
    assert int((a + b).max()) <= wc.MAX_EXP_SUM and int(a.max()) + int(b.max()) <= wc.MAX_EXP_SUM
    assert 3 * n * h * w * 2 ** wc.MAX_EXP_SUM < 2 ** 24
    assert torch.equal(x, x0 * (live * 2.0 ** b).unsqueeze(1)) and torch.equal(dy, dy0 * (live * 2.0 ** a).unsqueeze(1))
    assert torch.equal(x.bfloat16().float(), x) and torch.equal(dy.bfloat16().float(), dy)
    _assert_fp16_at_block_scale(x, "x"), _assert_fp16_at_block_scale(dy, "dy")
    for t in (dw, db):
        assert t.dtype == torch.float64 and torch.equal(t, t.round()) and 0 < float(t.abs().max()) < 2 ** 24


def test_random_operands():
    shape = wc.BF16_LONG[2]
    x, dy, ref64, ref32 = wc.random_case(shape, True)
    assert torch.equal(x.bfloat16().float(), x) and torch.equal(dy.bfloat16().float(), dy)
    assert 0.35 < float((x == 0).float().mean()) < 0.45
    assert ref64[0].dtype == torch.float64 and ref32[0].dtype == torch.float32
    e = wc.rel_err(ref32[0], ref64[0])
    assert 0 < e[1] < 1e-4, e      # the comparator is an fp32 computation of the same values: close to, not equal to, float64
    x2, _ = wc.random_operands(shape, False)
    assert not torch.equal(x2.bfloat16().float(), x2)
