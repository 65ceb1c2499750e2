"""CPU: precision 'bf16w2' (bf16 activations x two-piece bf16 weights, OSVOS_FLAG_BF16_W2) -- the Python and C-ABI surface that needs no GPU,
and a numpy restatement of the weight split that the GPU pack test (tests/test_gpu_bf16w2.py) compares the kernel's bytes against.

The split (include/osvos_hip.h, OSVOS_FLAG_BF16_W2): w_hi = RNE_bf16(w), w_lo = RNE_bf16(w - float(w_hi)), the subtraction exact in fp32."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W2 = 0x4000
BF16MFMA = 2
# (Cout, Cin as packed) of the 17 forward convolutions in wbuf order: 13 trunk (conv1_1 reads the 8-channel padded input), 4 side_prep
NET_LAYERS = [(64, 8), (64, 64), (128, 64), (128, 128), (256, 128), (256, 256), (256, 256), (512, 256), (512, 512), (512, 512),
              (512, 512), (512, 512), (512, 512), (16, 128), (16, 256), (16, 512), (16, 512)]


# precision -> the dtype words of (osvos_net_wbuf_bytes, osvos_net_pack, osvos_net_forward, osvos_net_backward), without OSVOS_FLAG_GENERIC_DECONV
DTYPE_WORDS = {"fp32": (0x0, 0x0, 0x0, 0x0), "bf16": (0x2, 0x2, 0x2, 0x2), "fp32x3": (0x3, 0x3, 0x3, 0x3), "fp32x2": (0x3, 0x3, 0x803, 0x803),
               "fp32x3b2": (0x3, 0x3, 0x3, 0x803), "fp32h2": (0x3, 0x3003, 0x1003, 0x1003), "fp32x3h2": (0x3, 0x2003, 0x3, 0x1003),
               "bf16w2": (0x4002, 0x4002, 0x4002, 0x2)}


# ---- numpy restatement of the split ------------------------------------------------------------------------------------------------------------
def rne_bf16(f32):
    """fp32 -> bf16 bits, round to nearest even; NaN stays NaN (quiet bit set); overflow rounds to +-inf -- csrc/common.h f32_to_bf16"""
    u = np.ascontiguousarray(f32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, ((u >> 16) | 0x40) & 0xFFFF, r)
    return r.astype(np.uint16)


def bf16_to_f32(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def split_w2(w):
    """(hi bits, lo bits) of fp32 weights; denormal fp32 operands and results are KEPT (no flush), as the pack kernel computes them"""
    w = np.ascontiguousarray(w, dtype=np.float32)
    hi = rne_bf16(w)
    with np.errstate(invalid="ignore", over="ignore"):
        lo = rne_bf16((w - bf16_to_f32(hi)).astype(np.float32))
    return hi, lo


def pack_w2_numpy(w_oihw):
    """the two-piece forward pack [plane][9][CinP/8][CoutP][8] as uint16 (CinP = Cin rounded up to 32, CoutP = Cout rounded up to 32, zero filled)"""
    cout, cin = w_oihw.shape[:2]
    cinp, coutp = (cin + 31) // 32 * 32, (cout + 31) // 32 * 32
    hi, lo = split_w2(w_oihw.reshape(cout, cin, 9))
    out = np.zeros((2, 9, cinp // 8, coutp, 8), dtype=np.uint16)
    for p, v in enumerate((hi, lo)):
        t = np.zeros((coutp, cinp, 9), dtype=np.uint16)
        t[:cout, :cin] = v
        out[p] = t.transpose(2, 1, 0).reshape(9, cinp // 8, 8, coutp).transpose(0, 1, 3, 2)
    return out


def test_split_error_bound_for_normal_weights():
    rng = np.random.default_rng(5)
    e = rng.uniform(-100, 60, 200000)
    w = (rng.choice([-1.0, 1.0], e.size) * rng.uniform(1.0, 2.0, e.size) * 2.0 ** e).astype(np.float32)
    hi, lo = split_w2(w)
    got = bf16_to_f32(hi).astype(np.float64) + bf16_to_f32(lo).astype(np.float64)
    err = np.abs(w.astype(np.float64) - got)
    keep = np.abs(w) >= 2.0 ** -100
    assert keep.sum() > 190000
    assert bool((err[keep] <= 2.0 ** -16 * np.abs(w[keep].astype(np.float64))).all()), float((err[keep] / np.abs(w[keep])).max())
    # the subtraction w - hi is exact in fp32: w == hi + r with r the fp32 difference, bit for bit
    r = (w - bf16_to_f32(hi)).astype(np.float32)
    assert bool((bf16_to_f32(hi).astype(np.float64) + r.astype(np.float64) == w.astype(np.float64)).all())
    # hi is plain RNE to bf16 -- the single-piece pack's value -- and lo is small next to it
    assert bool((np.abs(bf16_to_f32(lo)) <= 2.0 ** -8 * np.abs(bf16_to_f32(hi)) * 1.0001).all())


def test_split_edges_signed_zero_tiny_huge_ties_nan():
    def one(x):
        hi, lo = split_w2(np.array([x], dtype=np.float32))
        return int(hi[0]), int(lo[0])
    assert one(0.0) == (0x0000, 0x0000)
    assert one(-0.0) == (0x8000, 0x0000)            # -0 - (-0) = +0 under round to nearest
    # ties to even on the hi piece: 1 + 2^-8 is halfway between bf16 1.0 and 1 + 2^-7 -> 1.0, lo carries the 2^-8 exactly
    assert one(1.0 + 2.0 ** -8) == (0x3F80, 0x3B80)
    # 1 + 3 * 2^-8: halfway between 1 + 2^-7 (odd) and 1 + 2^-6 (even) -> up to the even one, lo = -2^-8
    assert one(1.0 + 3 * 2.0 ** -8) == (0x3F82, 0xBB80)
    # below 2^-100 the lo piece may leave the normal range: it is KEPT as a bf16 denormal (no flush), as is a denormal weight
    x = np.float32(2.0 ** -120 * (1 + 2.0 ** -9 + 2.0 ** -20))
    hi, lo = one(x)
    assert bf16_to_f32(np.array([hi]))[0] == np.float32(2.0 ** -120)
    assert lo != 0 and (lo & 0x7F80) == 0            # a denormal bf16, not zero
    d = np.float32(2.0 ** -130)                     # fp32 denormal that bf16 holds exactly (its denormals reach down to 2^-133)
    assert one(d) == (int(rne_bf16(np.array([d]))[0]), 0x0000) and one(d)[0] != 0
    # huge: FLT_MAX rounds to +inf in bf16, the residual is then -inf (what the spec's formula gives; no real weight is near it)
    assert one(np.finfo(np.float32).max) == (0x7F80, 0xFF80)
    big = np.float32(2.0 ** 127 * 1.5)
    assert one(big) == (0x7F40, 0x0000)
    assert one(np.inf) == (0x7F80, 0xFFC0)           # inf - inf = NaN: the lo piece of an infinite weight is a NaN
    hi, lo = one(np.nan)
    assert (hi & 0x7F80) == 0x7F80 and (hi & 0x7F) != 0 and (lo & 0x7F80) == 0x7F80 and (lo & 0x7F) != 0


def test_pack_layout_restatement_plane0_is_the_single_piece_pack():
    rng = np.random.default_rng(1)
    w = rng.standard_normal((40, 3, 3, 3)).astype(np.float32)
    p = pack_w2_numpy(w)
    assert p.shape == (2, 9, 4, 64, 8)
    # plane 0 entry (tap, cg, co, e) = RNE_bf16(W[co][8 cg + e][tap]); padding is zero in both planes
    assert p[0, 4, 0, 7, 2] == rne_bf16(w[7, 2, 1, 1:2])[0]
    assert p[1, 4, 0, 7, 2] == split_w2(w[7, 2, 1, 1:2])[1][0]
    assert not p[:, :, :, 40:].any() and not p[:, :, 0, :, 3:].any() and not p[:, :, 1:].any()


# ---- Python / C-ABI surface ---------------------------------------------------------------------------------------------------------------------
def test_precision_is_registered():
    from osvos_pytorch_amd.autograd import PRECISIONS
    from osvos_pytorch_amd._lib import BF16_W2, F32_BF16MFMA
    assert "bf16w2" in PRECISIONS and PRECISIONS["bf16w2"][0] == F32_BF16MFMA
    assert BF16_W2 == W2


def test_new_symbols_are_exported_and_bound():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    for name in ("osvos_conv3x3_bf16w2_fused", "osvos_conv3x3_bf16w2_tiles"):
        assert name in _lib.PROTOTYPES and hasattr(l, name), name
    import ctypes
    buf = (ctypes.c_int * 16)()
    n = l.osvos_conv3x3_bf16w2_tiles(buf, 16)
    tiles = [buf[i] for i in range(n)]
    assert tiles == list(range(40, 46))
    buf = (ctypes.c_int * 64)()
    single = [buf[i] for i in range(l.osvos_conv3x3_bf16io_tiles(buf, 64))]
    assert not set(tiles) & set(single)          # no tile id is both a single-piece and a two-piece kernel


def test_wbuf_grows_by_the_17_forward_lo_planes():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    planes = [l.osvos_wpack_bytes(co, ci, BF16MFMA) for co, ci in NET_LAYERS]
    assert all(p % 256 == 0 for p in planes)
    assert l.osvos_net_wbuf_bytes(BF16MFMA | W2) == l.osvos_net_wbuf_bytes(BF16MFMA) + sum(planes)
    assert 28e6 < sum(planes) < 31e6
    # the generic-head flag composes with it
    assert l.osvos_net_wbuf_bytes(BF16MFMA | W2 | 0x100) == l.osvos_net_wbuf_bytes(BF16MFMA | 0x100) + sum(planes)


def test_two_piece_pack_is_twice_the_single_piece_pack():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    for co, ci in NET_LAYERS + [(16, 16), (33, 40), (512, 3)]:
        assert l.osvos_wpack_bytes(co, ci, BF16MFMA | W2) == 2 * l.osvos_wpack_bytes(co, ci, BF16MFMA), (co, ci)


@pytest.mark.parametrize("dtype", [0, 3])
def test_flag_with_another_dtype_is_an_argument_error(dtype):
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    assert l.osvos_net_wbuf_bytes(dtype | W2) == 0
    assert b"BF16_W2" in l.osvos_last_error()
    assert l.osvos_wpack_bytes(64, 64, dtype | W2) == 0
    assert b"BF16_W2" in l.osvos_last_error()
    # the check comes before anything is launched: with null pointers and no stream the call still reports the flag, not a crash
    rc = l.osvos_pack_conv3x3_fwd(None, None, 64, 64, dtype | W2, None)
    assert rc < 0 and b"BF16_W2" in l.osvos_last_error()
    assert l.osvos_net_wbuf_bytes(dtype) > 0      # (the plain dtype is still fine)


def test_op_level_entry_refuses_bad_arguments_without_a_gpu():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    rc = l.osvos_conv3x3_bf16w2_fused(None, None, None, None, None, None, None, None, 1, 8, 8, 64, 64, 1, 0, None, -1, None)
    assert rc < 0 and b"y_bf16" in l.osvos_last_error()


def test_pack_format_is_part_of_the_pack_key():
    """the stale-pack hole: a precision switch that changes the pack format must change the key a graph recorded at its forward"""
    from osvos_pytorch_amd.autograd import PRECISIONS, NetRuntime
    rt = NetRuntime()
    fmts = {}
    for name in ("fp32", "fp32x3", "fp32x3b2", "fp32x2", "fp32x3h2", "fp32h2", "bf16", "bf16w2"):
        rt.set_precision(name)
        fmts[name] = rt.pack_format()
        # the four dtype words of the precision (wbuf, pack, forward, backward), composed in one place: autograd.Precision
        p = PRECISIONS[name]
        assert (p.wbuf_word(), p.pack_word(), p.fwd_word(), p.bwd_word()) == DTYPE_WORDS[name], name
        assert (rt.cdtype_fwd(), rt.cdtype_bwd(), rt.cdtype()) == (p.fwd_word(), p.bwd_word(), p.dtype) and rt.pack_format() == p.pack_format()
        rt.generic_head = True          # the generic-head flag is OR-ed into the words of the calls
        assert (rt.cdtype_fwd(), rt.cdtype_bwd(), rt.cdtype()) == (p.fwd_word() | 0x100, p.bwd_word() | 0x100, p.dtype | 0x100)
        rt.generic_head = False
    assert fmts["fp32x3"] == fmts["fp32x3b2"] == fmts["fp32x2"]        # same packs: no re-pack, a graph may cross these switches
    assert len({fmts[k] for k in ("fp32", "fp32x3", "fp32x3h2", "fp32h2", "bf16", "bf16w2")}) == 6
    # bf16 -> bf16w2 drops the buffer (it grows by the lo planes) and the key; the way back too
    rt.set_precision("bf16")
    rt.wbuf, rt.key = object(), (rt.pack_format(), ())
    rt.set_precision("bf16w2")
    assert rt.wbuf is None and rt.key is None and rt.cdtype_fwd() & W2 and not rt.cdtype_bwd() & W2
    rt.wbuf, rt.key = object(), (rt.pack_format(), ())
    rt.set_precision("bf16")
    assert rt.wbuf is None and rt.key is None and not rt.cdtype_fwd() & W2


def test_entry_scripts_offer_the_precision():
    from osvos_pytorch_amd.autograd import PRECISIONS, TEST_PRECISIONS
    # the scripts take their choices from the two tables: what the tables offer is pinned here
    assert sorted(PRECISIONS) == sorted(["fp32", "fp32x3", "fp32x3b2", "fp32x3h2", "fp32h2", "fp32x2", "bf16", "bf16w2"])
    assert sorted(TEST_PRECISIONS) == sorted(["fp32", "fp32x3", "fp32h2", "bf16", "bf16w2"])
    for script, opts in (("train_parent.py", {"--precision": "choices=list(PRECISIONS)"}),
                         ("train_online.py", {"--precision": "choices=list(PRECISIONS)", "--test-precision": "choices=[''] + list(TEST_PRECISIONS)"})):
        src = open(os.path.join(REPO, script)).read()
        for o, choices in opts.items():
            line = [l for l in src.splitlines() if "add_argument('%s'" % o in l]
            assert line and choices in line[0], (script, o)
        out = subprocess.run([sys.executable, os.path.join(REPO, script), "--help"], capture_output=True, text=True, timeout=300, cwd=REPO)
        assert out.returncode == 0, out.stderr[-2000:]
        for o in opts:      # the option's own choice list in the usage text names the precision
            usage = out.stdout.split("[" + o + " {", 1)
            assert len(usage) == 2 and "bf16w2" in usage[1].split("}", 1)[0].split(","), (script, o, out.stdout[:2000])
