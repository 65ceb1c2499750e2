"""CPU: the rule of osvos_lucid_compose_ex (deformation field, occluder, void band) as tests/lucid_deform_cases.py restates it -- the
vectorised restatement against the naive per-pixel loop and the brute-force band, the identity with tests/lucid_cases.py, the band's exact
properties -- and what runs without a GPU of osvos_pytorch_amd.lucid (check_lucid, field_shape) and of the --lucid-deform / --lucid-occlude /
--lucid-band rules of train_online.py.  LucidDream.draw cannot be reached without a device (the constructor inpaints and reads the box back):
its draw order and counts are pinned in tests/test_gpu_lucid_deform.py against lucid_deform_cases.draw.  The GPU tests compare the kernels
against this restatement bit for bit."""
import random

import numpy as np
import pytest

import lucid_cases as lc
import lucid_deform_cases as ld


def _same(got, want):
    return np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("h,w,mask,params,n,field,cell,occ,band", [
    (5, 7, "blob", "identity", 1, "noise", 8, "inside", 1), (4, 3, "checker", "mixed", 3, "smooth", 8, "mixed", 2),
    (1, 1, "full", "identity", 1, "max", 8, "rx0", 16), (9, 11, "blob", "rot30_s075", 1, "noise", 8, "partly_out", 3),
    (9, 11, "corner", "mixed", 2, "min", 16, "none", 0), (6, 9, "blob", "tone_high", 1, "none", 64, "whole", 1),
    (7, 10, "blob", "mirror", 1, "zero", 8, "none", 4)])
def test_restatement_equals_the_naive_loop(h, w, mask, params, n, field, cell, occ, band):
    bgr, bg, m = lc.frame_of("noise", h, w, 5), lc.frame_of("gradient", h, w), lc.mask_of(mask, h, w)
    M, tone = lc.params_of(params, h, w, n)
    D, o = ld.field_of(field, n, h, w, cell), ld.occluders_of(occ, n, h, w)
    assert _same(ld.compose_ex(bgr, m, bg, M, tone, o, D, cell, band), ld.compose_ex_naive(bgr, m, bg, M, tone, o, D, cell, band))


@pytest.mark.parametrize("c", lc.COMPOSE_CASES[:12], ids=lc.case_id)
def test_everything_off_is_the_plain_composition_word_for_word(c):
    """no field (or a zero field), no occluder (or rx = 0), band 0: lucid_cases.compose"""
    r = lc.compose_reference(c)
    h, w, n = c[0], c[1], c[4]
    args = (r["bgr"], r["mask"], r["bg"], r["M"], r["tone"])
    assert _same(ld.compose_ex(*args), (r["image"], r["gt"]))
    assert _same(ld.compose_ex(*args, occ=ld.occluders_of("rx0", n, h, w), D=ld.field_of("zero", n, h, w, 8), cell=8), (r["image"], r["gt"]))


def test_displacement_is_the_control_point_on_the_lattice_and_constant_fields_shift():
    h, w, cell = 20, 37, 8
    D = ld.field_of("noise", 1, h, w, cell)[0]
    dX, dY = ld.displacement(D, cell, h, w)
    assert np.array_equal(dX[::cell, ::cell], D[:(h - 1) // cell + 1, :(w - 1) // cell + 1, 0].astype(np.int64))
    assert np.array_equal(dY[::cell, ::cell], D[:(h - 1) // cell + 1, :(w - 1) // cell + 1, 1].astype(np.int64))
    # halfway between two control points: the rounded mean, half up (arithmetic shift)
    assert dX[0, 4] == (int(D[0, 0, 0]) + int(D[0, 1, 0]) + 1) >> 1
    # a constant field of whole pixels is an integer shift of the foreground: the same as the shift in the matrix
    bgr, bg, m = lc.frame_of("noise", h, w, 6), lc.frame_of("gradient", h, w), lc.mask_of("blob", h, w)
    const = np.zeros((1,) + ld.field_shape(h, w, cell) + (2,), np.int16)
    const[..., 0], const[..., 1] = 3 * 32, -2 * 32
    moved = [[[1.0, 0.0, 3.0, 0.0, 1.0, -2.0], lc.IDENTITY]]
    tone = [[lc.NEUTRAL, lc.NEUTRAL]]
    assert _same(ld.compose_ex(bgr, m, bg, [[lc.IDENTITY, lc.IDENTITY]], tone, D=const, cell=cell), lc.compose(bgr, m, bg, moved, tone))
    for v, cell in ((32767, 256), (-32768, 256), (-32768, 8)):      # the extreme sums stay inside int32 (asserted in displacement)
        full = np.full(ld.field_shape(h, w, cell) + (2,), v, np.int16)
        assert (ld.displacement(full, cell, h, w)[0] == v).all()


def test_occluder_shows_the_displaced_background_and_clears_the_label():
    h, w = 13, 17
    bgr, bg, m = lc.frame_of("noise", h, w, 6), lc.frame_of("gradient", h, w), lc.mask_of("full", h, w)
    occ = np.asarray([[8, 6, 4, 3, 2, -1]], np.int32)
    image, gt = ld.compose_ex(bgr, m, bg, [[lc.IDENTITY, lc.IDENTITY]], [[lc.NEUTRAL, lc.NEUTRAL]], occ=occ, mean=(0.0, 0.0, 0.0))
    cov = ld.covered(occ[0], h, w)
    assert cov[6, 8] and cov[6, 4] and cov[6, 12] and not cov[6, 3] and cov[3, 8] and not cov[2, 8] and not cov[4, 5] and 0 < cov.sum() < h * w
    assert np.array_equal(gt[0, 0], (~cov).astype(np.float32))
    yy, xx = np.nonzero(cov)
    want = bg[np.clip(yy - 1, 0, h - 1), np.clip(xx + 2, 0, w - 1)].astype(np.float32)
    assert np.array_equal(image[0][:, yy, xx].T, want) and np.array_equal(image[0][:, ~cov].T, bgr[~cov].astype(np.float32))
    assert not ld.covered((8, 6, 0, 3, 0, 0), h, w).any() and not ld.covered((8, 6, 4, 0, 0, 0), h, w).any()
    assert ld.covered((8, 6, 4096, 4096, 0, 0), h, w).all()


@pytest.mark.parametrize("band", [1, 2, 5, 16])
@pytest.mark.parametrize("h,w,kind", [(7, 10, "blob"), (9, 9, "ring"), (5, 12, "checker"), (12, 6, "corner"), (1, 1, "full"), (6, 8, "dots")])
def test_band_equals_the_brute_force_loop(h, w, kind, band):
    L = lc.mask_of(kind, h, w) != 0
    assert np.array_equal(ld.void_band(L, band), ld.void_band_brute(L, band))


def test_band_properties():
    h, w = 21, 30
    for band in (1, 3, 16):
        for uniform in (np.zeros((h, w), bool), np.ones((h, w), bool)):      # a uniform plane has no edge: the image border is none
            assert not ld.void_band(uniform, band).any()
    L = np.zeros((h, w), bool)
    L[:, 15:] = True                                                          # one straight edge between columns 14 and 15
    for band in (1, 3, 7):
        v = ld.void_band(L, band)
        assert np.array_equal(v, np.broadcast_to((np.arange(w) >= 15 - band) & (np.arange(w) < 15 + band), (h, w)))      # symmetric across it
        assert np.array_equal(v, ld.void_band(~L, band))                                                                # and under exchange
    # a disc, not a square: (3, 3) away is outside band 4 (18 > 16), (0, 4) away is inside
    L = np.zeros((h, w), bool)
    L[10, 10] = True
    v = ld.void_band(L, 4)
    assert v[10, 14] and v[14, 10] and v[10, 10] and not v[13, 13] and v[12, 13] and not v[10, 15]
    # a band wider than the image on a mixed plane voids everything
    L = lc.mask_of("corner", 5, 12) != 0
    assert L.any() and not L.all() and ld.void_band(L, 16).all()
    gt = ld.reference((5, 70, "edge64", "identity", 1, "none", 64, "none", 1))["gt"][0, 0]
    assert (gt[:, 62:66] == [1, -1, -1, 0]).all() and (gt[:, :63] == 1).all() and (gt[:, 65:] == 0).all()


def test_check_lucid_limits_and_field_shape():
    from osvos_pytorch_amd import _lib, lucid
    assert (_lib.LUCID_MAX_BAND, _lib.LUCID_MIN_CELL, _lib.LUCID_MAX_CELL) == (ld.MAX_BAND, ld.MIN_CELL, ld.MAX_CELL) == (16, 8, 256)
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "osvos_hip.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define OSVOS_LUCID_(MAX_BAND|MIN_CELL|MAX_CELL|MAX_OCC_RADIUS|MAX_OCC_OFFSET)\s+(\d+)", hdr)}
    assert got == dict(MAX_BAND=16, MIN_CELL=8, MAX_CELL=256, MAX_OCC_RADIUS=_lib.LUCID_MAX_OCC_RADIUS, MAX_OCC_OFFSET=_lib.LUCID_MAX_OCC_OFFSET)
    assert (got["MAX_OCC_RADIUS"], got["MAX_OCC_OFFSET"]) == (4096, 8192)
    lucid.check_lucid(deform=0.0, occlude=0.0, band=0, cell=8)
    lucid.check_lucid(deform=1.0, occlude=1.0, band=16, cell=256)
    lucid.check_lucid(0.5, 5, 2, 3, 0.25, 0.05, 0.2, 20, 0.5, 0.5, 3, 16)
    for bad in [dict(deform=-0.1), dict(deform=1.5), dict(deform=float("nan")), dict(deform=None), dict(occlude=-0.1), dict(occlude=1.01),
                dict(occlude="1"), dict(band=-1), dict(band=17), dict(band=2.0), dict(band=True), dict(cell=4), dict(cell=512), dict(cell=24),
                dict(cell=0), dict(cell=64.0)]:
        with pytest.raises(ValueError):
            lucid.check_lucid(**bad)
    for h, w, cell in [(1, 1, 8), (37, 53, 8), (37, 53, 64), (480, 854, 128), (64, 64, 64), (65, 65, 64), (5, 257, 256)]:
        assert lucid.field_shape(h, w, cell) == ld.field_shape(h, w, cell) == ((h - 1) // cell + 2, (w - 1) // cell + 2)
    for bad in [(0, 5, 8), (5, 5, 12), (5, 5, 4)]:
        with pytest.raises(ValueError):
            lucid.field_shape(*bad)
    import inspect
    p = inspect.signature(lucid.LucidDream.__init__).parameters
    assert [p[k].default for k in ("deform", "deform_cell", "occlude", "band")] == [0.0, 128, 0.0, 0]
    p = inspect.signature(lucid.compose).parameters
    assert [p[k].default for k in ("occluders", "field", "cell", "band", "ws")] == [None, None, 64, 0, None]


def test_restated_draws_take_their_numbers_in_the_documented_order():
    """lucid_deform_cases.draw (what the GPU test holds LucidDream.draw to): counts and order"""
    h, w, cell = 37, 53, 16
    gh, gw = ld.field_shape(h, w, cell)
    box = (10, 29, 5, 14)
    for deform, occlude, count in ((0.0, 0.0, 0), (0.5, 0.0, 2 * gh * gw), (0.0, 0.7, 7), (0.5, 1.0, 2 * gh * gw + 7)):
        random.seed(5)
        field, occ = ld.draw(random.random, box, h, w, deform, cell, occlude)
        state = random.getstate()
        random.seed(5)
        u = [random.random() for _ in range(count)]
        assert random.getstate() == state
        if deform:
            assert field.shape == (gh, gw, 2) and field[0, 0, 1] == round(4 * cell * deform * (2 * u[1] - 1)) and np.abs(field).max() <= 4 * cell * deform
            assert field[1, 2, 0] == round(4 * cell * deform * (2 * u[2 * (gw + 2)] - 1))
        else:
            assert field is None
        if occlude == 1.0:
            v = u[2 * gh * gw:]
            assert occ == [round(10 + v[1] * 20), round(5 + v[2] * 10), round((0.1 + 0.2 * v[3]) * 20), round((0.1 + 0.2 * v[4]) * 10),
                           round((2 * v[5] - 1) * w / 4), round((2 * v[6] - 1) * h / 4)]
    random.seed(5)
    assert ld.draw(random.random, None, h, w, 0.0, cell, 1.0)[1] == [0] * 6            # an empty mask: rx = 0, seven numbers all the same
    assert ld.draw(lambda: 0.9, box, h, w, 0.0, cell, 0.5)[1] == [0] * 6               # absent


def test_deform_flags_are_parsed_and_refused_before_gpu_work():
    import train_online
    base = ["--synthetic", "--device-augment"]
    plain = dict(p=0.5, fg_shift=0.25, bg_shift=0.05, gain=0.2, offset=20, **lc.DEFAULTS)
    a = train_online.parse_args(base + ["--lucid", "0.5", "--lucid-deform", "0.5,16", "--lucid-occlude", "0.25", "--lucid-band", "3"])
    assert a.lucid == dict(plain, deform=0.5, deform_cell=16, occlude=0.25, band=3) and a.lucid_void is True
    a = train_online.parse_args(base + ["--lucid", "0.5", "--lucid-deform", "1"])
    assert a.lucid == dict(plain, deform=1.0, deform_cell=128) and a.lucid_void is False
    a = train_online.parse_args(base + ["--multi-object", "--lucid", "0.5", "--lucid-band", "16"])
    assert a.lucid == dict(plain, band=16) and a.lucid_void is True
    # off: the keyword arguments of before, nothing more
    a = train_online.parse_args(base + ["--lucid", "0.5", "--lucid-deform", "0", "--lucid-occlude", "0", "--lucid-band", "0"])
    assert a.lucid == plain and a.lucid_void is False
    a = train_online.parse_args(base + ["--lucid-deform", "0.5", "--lucid-band", "3"])      # without --lucid nothing is built
    assert a.lucid is None and a.lucid_void is False
    bad = [(base + ["--lucid-deform", "1.5"], "deform"), (base + ["--lucid-deform", "-1"], "deform"), (base + ["--lucid-deform", "0.5,24"], "cell"),
           (base + ["--lucid-deform", "0.5,4"], "cell"), (base + ["--lucid-deform", "0.5,512"], "cell"), (base + ["--lucid-deform", "0.5,16,2"], "--lucid-deform"),
           (base + ["--lucid-deform", "x"], "--lucid-deform"), (base + ["--lucid-deform", "0.5,8.5"], "--lucid-deform"),
           (base + ["--lucid-occlude", "1.5"], "occlude"), (base + ["--lucid-occlude", "-0.5"], "occlude"), (base + ["--lucid-band", "17"], "band"),
           (base + ["--lucid-band", "-1"], "band"), (base + ["--lucid", "0.5", "--lucid-band", "3", "--window-fused"], "--window-fused"),
           (["--synthetic", "--lucid", "0.5", "--lucid-band", "3"], "--device-augment")]
    for argv, word in bad:
        with pytest.raises(SystemExit) as e:
            train_online.parse_args(argv)
        assert word in str(e.value), (argv, e.value)
    assert train_online.parse_args(base + ["--lucid", "0.5", "--window-fused"]).lucid == plain      # band 0 still combines


def test_band_without_the_fused_loss_is_refused_before_the_library_is_loaded():
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, train_online\n"
            "for argv in (['--lucid', '0.5', '--lucid-band', '3'], ['--lucid-deform', '2']):\n"
            "    try:\n"
            "        train_online.parse_args(['--synthetic', '--device-augment'] + argv)\n"
            "        sys.exit(3)\n"
            "    except SystemExit as e:\n"
            "        assert '--lucid' in str(e) and ('fused loss' in str(e) or 'deform' in str(e)), e\n"
            "assert train_online.parse_args(['--synthetic', '--device-augment', '--lucid', '0.5']).lucid_void is False\n"
            "from osvos_pytorch_amd import _lib\n"
            "assert _lib._lib is None\n"
            "print('refused before the library')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=repo, env=dict(os.environ, PYTHONPATH=repo, OSVOS_FUSED_LOSS_STEP="0"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "refused before the library" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]
