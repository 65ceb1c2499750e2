"""The persistent bf16 convolutions with SEVERAL tiles per workgroup: conv3x3_bf16_p64.hip (tiles 38 / 138) and the persistent LDS-DMA forms of
conv3x3_bf16_dma.hip (34-37, 134-137).  What makes these kernels delicate -- the pending register set and its tile cursor, the mask words and pool
rows of the pending tile, the `s_waitcnt vmcnt` budgets of a workgroup's second and later tiles, the stepped cursor's carries, the dead tail tiles
of map 2, the issue side running ahead across tile boundaries -- only happens from a workgroup's second tile on, and the op tests of
test_gpu_ops.py give every workgroup one tile.

Part 1 (library as shipped, no switch): a tile's K order and epilogue depend neither on the image index nor on the workgroup that runs it, so image n
of a batch-N launch must equal BIT FOR BIT the single-image launch of x[n:n+1] on the same tile id -- and a single-image launch of these shapes is
one tile per workgroup, the path test_conv3x3_bf16act_fused_epilogues_every_tile pins against float64.  The batch results are also held against
float64 and against the separate pooling kernel themselves, so that a wrong single-image launch cannot hide.  The test computes the block count and
the persistent grid from the geometry written here and the device's CU count and ASSERTS that the single-image launch has one tile per workgroup and
the batch launch at least three (phase 2 of the wait budgets); on a device where that does not hold it fails and names the batch size that would.

Part 2 (OSVOS_P64_GRID / OSVOS_DMA_GRID: -1 = one tile per workgroup, 0 = shipped grid, 16 = sixteen workgroups with ~50 tiles each): all three
grids must give the same bits in every output of every mode, on the production launches the per-image oracle cannot split (conv1_2 at batch 2,
conv2_1 at batch 12, 854x480) and on two of the small shapes.  The switches are read once per process, so each arm is a child process.

A miscounted vmcnt is a race: it shows as a bit mismatch only when a DMA is actually late.  Random per-tile data makes any stale slot visible and
the maps and grids vary the timing, but a pass is evidence, not proof."""
import functools
import hashlib
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tile id % 100 -> (tile rows, couts per cout tile, resident filter); every tile is 32 pixels wide.  34-37: DmaCfg variants 4-7 of conv3x3_bf16_dma.hip
# (<4, 2>, <4, 4>, <2, 4, 64>, <2, 2, 64>: TH = 4 WGM, BN = 32 NB), 38: TH / BN of conv3x3_bf16_p64.hip.  Tile ids >= 100 ask for the XCD-local block
# order: map 1 (eight consecutive blocks = eight spatial tiles) in the DMA kernels, map 2 (XCD k owns a contiguous band of spatial tiles) in tile 38.
GEOM = {34: (8, 128, False), 35: (16, 128, False), 36: (16, 64, True), 37: (8, 64, True), 38: (16, 64, True)}
TW = 32
TILES = [38, 138, 34, 134, 35, 135, 36, 136, 37, 137]

# (N, H, W, Cin, Cout), and the N of the kernels with 128-cout tiles where those halve the block count (256 CUs: >= 768 blocks wanted)
SHAPES = [
    ((24, 100, 140, 64, 64), 24),     # ragged last tile row and column; spatial stride digits (7, 2, 1) in map 0, (0, 6, 2) in map 2: both carries
    ((70, 37, 53, 64, 128), 140),     # two cout tiles, odd H and W (partial pool windows at tile and image edges), 4 dead tail tiles in map 2
    ((48, 48, 96, 64, 96), 96),       # second cout tile half empty (CoutP = 96: the co < Cout guards of every store)
    ((70, 50, 70, 64, 40), 70),       # Cout % 32 != 0: no one-bit masks (an argument error), plain and pool modes only
]


def _cdiv(a, b):
    return -(-a // b)


def _shape_for(shape, n128, tile):
    return ((n128 if GEOM[tile % 100][1] == 128 else shape[0]),) + tuple(shape[1:])


def _map_of(tile):
    return 0 if tile < 100 else (2 if tile % 100 == 38 else 1)


def _geometry(shape, tile, cus):
    """What the launchers compute: tiles per image, cout tiles, blocks, and the persistent grid of a device with `cus` compute units."""
    n, h, w, _, cout = shape
    th, bn, res = GEOM[tile % 100]
    nct = _cdiv(_cdiv(cout, 32) * 32, bn)
    ty, tx = _cdiv(h, th), _cdiv(w, TW)
    nsp = n * ty * tx
    band = _cdiv(nsp, 8)
    blocks = nct * nsp if tile < 100 else nct * band * 8
    gmul = 8 * (nct if res else 1)
    cu = cus if tile % 100 == 38 else max(cus // 8 * 8, 8)
    gmax = cu // gmul * gmul
    assert gmax > 0, (tile, cus)
    return dict(th=th, bn=bn, nct=nct, ty=ty, tx=tx, nsp=nsp, band=band, blocks=blocks, gmul=gmul, gmax=gmax, grid=min(blocks, gmax))


def _grid_of(geo, knob):
    if knob > 0:
        return min(geo["blocks"], max(geo["gmul"], knob // geo["gmul"] * geo["gmul"]))
    return geo["blocks"] if knob < 0 else geo["grid"]


def _where(geo, tile, grid, n, ty, tx, ct):
    """(workgroup, ordinal ti of the tile inside the workgroup's walk) of tile (image, tile row, tile column, cout tile)"""
    sp = (n * geo["ty"] + ty) * geo["tx"] + tx
    m = _map_of(tile)
    if m == 0:
        t = sp * geo["nct"] + ct
    elif m == 1:
        t = ((sp // 8) * geo["nct"] + ct) * 8 + sp % 8
    else:
        t = ((sp % geo["band"]) * geo["nct"] + ct) * 8 + sp // geo["band"]
    return t % grid, t // grid


def _bits_of(t_nhwc):
    """[N,H,W,C] -> int64 [N,H,W,C/32]: bit b of word g = (t[..., 32 g + b] > 0) (csrc/maskbits.h)"""
    n, h, w, c = t_nhwc.shape
    pos = (t_nhwc > 0).long().reshape(n, h, w, c // 32, 32)
    return (pos << torch.arange(32, device=t_nhwc.device)).sum(-1)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=1)
def _problem(shape, images=None):
    """bf16-representable x and w, bias 0.1 randn, a random mask; float64 references (NHWC, on the GPU) of the images asked for (None = all)"""
    n, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(sum(shape) + 5)
    x = torch.randn(n, cin, h, w, generator=g).bfloat16()
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)).bfloat16().float()
    b = torch.randn(cout, generator=g) * 0.1
    m = torch.randn(n, cout, h, w, generator=g)
    sel = list(range(n)) if images is None else list(images)
    xs, ms = x[sel].double(), m[sel]
    ref = _nhwc(F.relu(F.conv2d(xs, wt.double(), b.double(), padding=1))).cuda()
    ref_masked = _nhwc(F.conv2d(xs, wt.double(), None, padding=1) * (ms > 0)).cuda()
    has_bits = cout % 32 == 0
    m_nhwc = _nhwc(m).cuda()
    return dict(x=_nhwc(x.float()).bfloat16().cuda(), wt=wt.cuda(), b=b.cuda(), m=m_nhwc, sel=sel, ref=ref, ref_masked=ref_masked,
                mbits=_bits_of(m_nhwc).to(torch.int32) if has_bits else None)      # (values >= 2^31 wrap to the same 32 bits)


def _launch_modes(ops, tile, x, wpk, b, cout, mbits):
    """Every mode of one tile id on one input: MODE 0 (result + sign bits), MODE 1 (result + fused pool + code bytes), the plain call, MODE 2 (masked
    data gradient).  Tile 38 takes sign bits and the pool in separate launches; the DMA tiles' epilogue gives both from one."""
    out = {}
    one = tile % 100 != 38
    if cout % 32 == 0:
        out["y"], out["bits"], p, c = ops.conv3x3_bf16act_fused(x, wpk, b, cout, relu=True, want_bits=True, want_pool=one, tile=tile)
        if one:
            out["y_pool"], out["pooled"], out["code"] = out["y"], p, c
    if "pooled" not in out:
        out["y_pool"], _, out["pooled"], out["code"] = ops.conv3x3_bf16act_fused(x, wpk, b, cout, relu=True, want_pool=True, tile=tile)
    out["y_plain"] = ops.conv3x3_bf16act_fused(x, wpk, b, cout, relu=True, tile=tile)[0]
    out.setdefault("y", out["y_plain"])
    if mbits is not None:
        out["dgrad"] = ops.conv3x3_bf16act_fused(x, wpk, None, cout, relu=False, mask_bits=mbits, tile=tile)[0]
    return out


def _within_bf16_of(y, ref):
    err = (y.double() - ref).abs()
    return float((err / (ref.abs() * 2.0 ** -8 + 1e-3)).max()), float(err.max())


def _check_batch_alone(ops, out, prob, cout, what):
    """the batch results against float64 and against the separate kernels (|err| <= |ref| 2^-8 + 1e-3: the bar of the every-tile op test)"""
    sel = prob["sel"]
    r, e = _within_bf16_of(out["y"][sel], prob["ref"])
    assert r <= 1.0, (what, "result vs float64", r, e)
    assert torch.equal(out["y"], out["y_pool"]) and torch.equal(out["y"], out["y_plain"]), (what, "the modes disagree on the result")
    p_ref, c_ref = ops.maxpool2x2_bf16act_code(out["y"])
    assert torch.equal(out["pooled"], p_ref), (what, "fused pool vs pooling kernel")
    assert torch.equal(out["code"], c_ref), (what, "pool code bytes vs pooling kernel")
    if cout % 32 == 0:
        assert torch.equal(_bits_of(out["y"].float()), out["bits"].long() & 0xFFFFFFFF), (what, "sign bits")
        r, e = _within_bf16_of(out["dgrad"][sel], prob["ref_masked"])
        assert r <= 1.0, (what, "masked data gradient vs float64", r, e)
        assert bool(((out["dgrad"] != 0) <= (prob["m"] > 0)).all()), (what, "gradient where the mask is <= 0")


def _bad_tiles(a, b, geo, tile, grid, scale):
    """tiles (image, tile row, tile column, cout tile) in which a and b [N,h,w,c] differ, with the workgroup and ordinal that ran them;
    scale = 2 for the pooled tensors; the last axis of the bit tensors is words of 32 couts"""
    cpt = geo["bn"] // 32 if a.dtype == torch.int32 else geo["bn"]
    th, tw = geo["th"] // scale, TW // scale
    idx = (a != b).nonzero()
    tiles = torch.stack([idx[:, 0], idx[:, 1] // th, idx[:, 2] // tw, idx[:, 3] // cpt], 1).unique(dim=0).tolist()
    return [(tuple(t), "wg %d ti %d" % _where(geo, tile, grid, *t)) for t in tiles]


def _require_unset():
    for k in ("OSVOS_P64_GRID", "OSVOS_DMA_GRID", "OSVOS_P64_BAND"):
        assert k not in os.environ, "%s is set: this test is about the library as shipped" % k


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("shape,n128", SHAPES, ids=["x".join(map(str, s)) for s, _ in SHAPES])
def test_batch_launch_equals_single_image_launches_bit_for_bit(shape, n128, tile):
    from osvos_pytorch_amd import ops
    from osvos_pytorch_amd._lib import F32_BF16MFMA
    _require_unset()
    shape = _shape_for(shape, n128, tile)
    n, h, w, cin, cout = shape
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    geo, geo1 = _geometry(shape, tile, cus), _geometry((1,) + shape[1:], tile, cus)
    need = _cdiv(3 * geo["gmax"], geo["blocks"] // n)
    # (a) a single image: one tile per workgroup; (b) the batch: every workgroup gets at least three tiles (phase 2 of the wait budgets)
    assert geo1["blocks"] <= geo1["gmax"], "%s tile %d on %d CUs: one image is %d blocks for a grid of %d -- the oracle itself is multi-tile" % (
        shape, tile, cus, geo1["blocks"], geo1["gmax"])
    assert geo["blocks"] >= 3 * geo["grid"], "%s tile %d on %d CUs: %d blocks for a grid of %d is under three tiles per workgroup; N >= %d restores it" % (
        shape, tile, cus, geo["blocks"], geo["grid"], need)
    prob = _problem(shape)
    wpk = ops.pack_fwd(prob["wt"], F32_BF16MFMA)
    what = (shape, tile, "map %d" % _map_of(tile), "grid %d" % geo["grid"])
    if cout % 32 != 0:      # one-bit masks need whole words per pixel
        bad_mask = torch.zeros(n, h, w, 1, dtype=torch.int32, device="cuda")
        with pytest.raises(RuntimeError):
            ops.conv3x3_bf16act_fused(prob["x"], wpk, prob["b"], cout, relu=True, want_bits=True, tile=tile)
        with pytest.raises(RuntimeError):
            ops.conv3x3_bf16act_fused(prob["x"], wpk, None, cout, relu=False, mask_bits=bad_mask, tile=tile)
    batch = _launch_modes(ops, tile, prob["x"], wpk, prob["b"], cout, prob["mbits"])
    assert set(batch) == ({"y", "bits", "y_pool", "pooled", "code", "y_plain", "dgrad"} if cout % 32 == 0 else {"y", "y_pool", "pooled", "code", "y_plain"})
    singles = [_launch_modes(ops, tile, prob["x"][i:i + 1], wpk, prob["b"], cout, None if prob["mbits"] is None else prob["mbits"][i:i + 1]) for i in range(n)]
    torch.cuda.synchronize()
    wrong = {}
    for k in sorted(batch):
        single = torch.cat([s[k] for s in singles])
        if not torch.equal(batch[k], single):
            bad = _bad_tiles(batch[k], single, geo, tile, geo["grid"], 2 if k in ("pooled", "code") else 1)
            wrong[k] = (len(bad), bad[:24])
            print("MISMATCH %s output %s: %d tiles (image, tile row, tile column, cout tile), the first: %s" % (what, k, len(bad), bad[:40]))
    assert not wrong, (what, wrong)
    _check_batch_alone(ops, batch, prob, cout, what)


# ---- part 2: the grid switches, one child process per arm

ARMS = (-1, 0, 16)
PRODUCTION = [((2, 480, 854, 64, 64), (38, 138), True),         # conv1_2 at batch 2: MODE 0, 1 and 2
              ((12, 240, 427, 64, 128), (38, 138), False)]      # conv2_1 at batch 12: MODE 0 and 2
SMALL = [SHAPES[0], SHAPES[1]]


def _digest(t, rows):
    """one hash per (image, band of `rows` rows) of [N,h,w,c]: equal digests <=> equal bits, and a mismatch names image and tile row"""
    raw = t.contiguous().cpu()
    raw = raw.view(torch.int16) if raw.dtype == torch.bfloat16 else raw
    return [[hashlib.blake2b(raw[i, r:r + rows].numpy().tobytes(), digest_size=16).digest() for r in range(0, raw.shape[1], rows)] for i in range(raw.shape[0])]


def _digests(out, tile):
    th = GEOM[tile % 100][0]
    return {k: _digest(v, th // 2 if k in ("pooled", "code") else th) for k, v in out.items()}


def _production_modes(ops, tile, prob, wpk, cout, pool):
    out = {}
    out["y"], out["bits"], _, _ = ops.conv3x3_bf16act_fused(prob["x"], wpk, prob["b"], cout, relu=True, want_bits=True, tile=tile)
    if pool:
        out["y_pool"], _, out["pooled"], out["code"] = ops.conv3x3_bf16act_fused(prob["x"], wpk, prob["b"], cout, relu=True, want_pool=True, tile=tile)
    out["dgrad"] = ops.conv3x3_bf16act_fused(prob["x"], wpk, None, cout, relu=False, mask_bits=prob["mbits"], tile=tile)[0]
    return out


def child_main(path):
    """what one arm computes (run in a child process with the two grid switches set): digests of every output of every case, and the float64 verdicts
    on the first and the last image of the production launches"""
    from osvos_pytorch_amd import ops
    from osvos_pytorch_amd._lib import F32_BF16MFMA
    res = {}
    for shape, tiles, pool in PRODUCTION:
        n, cout = shape[0], shape[4]
        prob = _problem(shape, (0, n - 1))
        wpk = ops.pack_fwd(prob["wt"], F32_BF16MFMA)
        for tile in tiles:
            out = _production_modes(ops, tile, prob, wpk, cout, pool)
            torch.cuda.synchronize()
            res["digest", shape, tile] = _digests(out, tile)
            res["bar", shape, tile] = (_within_bf16_of(out["y"][prob["sel"]], prob["ref"]), _within_bf16_of(out["dgrad"][prob["sel"]], prob["ref_masked"]))
            res["bits", shape, tile] = torch.equal(_bits_of(out["y"].float()), out["bits"].long() & 0xFFFFFFFF)
            res["masked", shape, tile] = bool(((out["dgrad"] != 0) <= (prob["m"] > 0)).all())
            if pool:
                p_ref, c_ref = ops.maxpool2x2_bf16act_code(out["y"])
                res["pool", shape, tile] = torch.equal(out["y"], out["y_pool"]) and torch.equal(out["pooled"], p_ref) and torch.equal(out["code"], c_ref)
            del out
    for base, n128 in SMALL:
        for tile in TILES:
            shape = _shape_for(base, n128, tile)
            prob = _problem(shape, (0, shape[0] - 1))
            wpk = ops.pack_fwd(prob["wt"], F32_BF16MFMA)
            out = _launch_modes(ops, tile, prob["x"], wpk, prob["b"], shape[4], prob["mbits"])
            torch.cuda.synchronize()
            res["digest", shape, tile] = _digests(out, tile)
            res["bar", shape, tile] = (_within_bf16_of(out["y"][prob["sel"]], prob["ref"]), _within_bf16_of(out["dgrad"][prob["sel"]], prob["ref_masked"]))
    torch.save(res, path)


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_persistent_tiles as t
t.child_main(sys.argv[2])
"""


@pytest.fixture(scope="module")
def arms(tmp_path_factory):
    """the three arms, one after the other; a child that fails ends the run (no further child is started)"""
    _require_unset()
    tmp = tmp_path_factory.mktemp("grid_arms")
    res = {}
    for knob in ARMS:
        path = str(tmp / ("arm_%d.pt" % knob))
        env = dict(os.environ, OSVOS_P64_GRID=str(knob), OSVOS_DMA_GRID=str(knob))
        r = subprocess.run([sys.executable, "-c", CHILD, REPO, path], env=env, cwd=REPO, capture_output=True, text=True, timeout=420)
        assert r.returncode == 0, ("grid %d" % knob, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        res[knob] = torch.load(path, weights_only=False)
    return res


def _differing(da, db, shape, tile, knob_a, knob_b):
    """(output, image, tile row, workgroups and ordinals of that row's first tile under either grid) where two arms' digests differ"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    geo = _geometry(shape, tile, cus)
    bad = []
    for k in sorted(da):
        for i, (ra, rb) in enumerate(zip(da[k], db[k])):
            for r, (ha, hb) in enumerate(zip(ra, rb)):
                if ha != hb:
                    bad.append((k, i, r, "grid %d: wg %d ti %d" % ((knob_a,) + _where(geo, tile, _grid_of(geo, knob_a), i, r, 0, 0)),
                                "grid %d: wg %d ti %d" % ((knob_b,) + _where(geo, tile, _grid_of(geo, knob_b), i, r, 0, 0))))
    return bad


def _cases():
    return [(s, t) for s, tiles, _ in PRODUCTION for t in tiles] + [(_shape_for(b, n128, t), t) for b, n128 in SMALL for t in TILES]


def test_grid_arms_cover_one_many_and_shipped_tiles_per_workgroup():
    """the three arms are what they are meant to be on this device: one tile per workgroup, the shipped grid with several, sixteen-odd workgroups"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for shape, tile in _cases():
        geo = _geometry(shape, tile, cus)
        assert _grid_of(geo, -1) == geo["blocks"]
        assert geo["blocks"] >= 2 * _grid_of(geo, 0), (shape, tile, geo)
        assert _grid_of(geo, 16) == geo["gmul"] * max(1, 16 // geo["gmul"]) and geo["blocks"] >= 40 * _grid_of(geo, 16), (shape, tile, geo)


def test_every_grid_gives_the_same_bits(arms):
    wrong = {}
    for shape, tile in _cases():
        ref = arms[0]["digest", shape, tile]
        for knob in (-1, 16):
            got = arms[knob]["digest", shape, tile]
            assert got.keys() == ref.keys()
            if got != ref:
                bad = _differing(ref, got, shape, tile, 0, knob)
                wrong[shape, tile, "map %d" % _map_of(tile), knob] = (len(bad), bad[:24])
                print("MISMATCH %s tile %d map %d, grid 0 vs %d: (output, image, tile row, where), %d in all, the first: %s" % (shape, tile, _map_of(tile), knob, len(bad), bad[:40]))
    assert not wrong, wrong


def test_every_grid_is_within_bf16_of_float64_on_first_and_last_image(arms):
    for knob in ARMS:
        for shape, tile in _cases():
            (ry, ey), (rd, ed) = arms[knob]["bar", shape, tile]
            assert ry <= 1.0 and rd <= 1.0, (knob, shape, tile, ry, ey, rd, ed)
        for shape, tiles, pool in PRODUCTION:
            for tile in tiles:
                assert arms[knob]["bits", shape, tile] and arms[knob]["masked", shape, tile], (knob, shape, tile)
                assert not pool or arms[knob]["pool", shape, tile], (knob, shape, tile)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("base,n128", SMALL, ids=["x".join(map(str, s)) for s, _ in SMALL])
def test_grid_switch_at_zero_is_the_shipped_library(arms, base, n128, tile):
    """with the switches at 0 the library launches the grids it launches without them: same bits as this (switch-free) process"""
    from osvos_pytorch_amd import ops
    from osvos_pytorch_amd._lib import F32_BF16MFMA
    _require_unset()
    shape = _shape_for(base, n128, tile)
    prob = _problem(shape, (0, shape[0] - 1))
    wpk = ops.pack_fwd(prob["wt"], F32_BF16MFMA)
    out = _launch_modes(ops, tile, prob["x"], wpk, prob["b"], shape[4], prob["mbits"])
    torch.cuda.synchronize()
    here = _digests(out, tile)
    assert here == arms[0]["digest", shape, tile], (shape, tile, _differing(here, arms[0]["digest", shape, tile], shape, tile, 0, 0)[:24])
