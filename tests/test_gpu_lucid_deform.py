"""GPU: osvos_lucid_compose_ex (csrc/lucid.hip) -- the composition with a deformation field, an occluder and a void band -- against the
numpy restatement of the rule in tests/lucid_deform_cases.py, bit for bit (integer arithmetic: every comparison is np.array_equal, there is
no tolerance); the identity with osvos_lucid_compose, the refusals, the size query, the wrappers of osvos_pytorch_amd.lucid, LucidDream with
the options, and train_online.py --lucid-deform / --lucid-occlude / --lucid-band.  Outputs and the workspace are pre-filled with garbage
before every call, and a guard region after the workspace must keep it."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import lucid_cases as lc
import lucid_deform_cases as ld
import script_runner

pytestmark = pytest.mark.gpu
GARBAGE_BYTE = 0xa5
GUARD = 256


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                       # (a copy: the shared references are read-only)


def _np(t):
    return t.cpu().numpy()


def _bits(t):
    return _np(t).view(np.uint32)


def _ex_rc(bgr, mask, bg, M, tone, occ=None, D=None, cell=64, band=0, mean=lc.MEAN, n=None, h=None, w=None, ws="own", ws_offset=0, d_offset=0):
    """one osvos_lucid_compose_ex call through _lib on CUDA tensors -> (rc, image, gt, ws buffer, ws bytes); bgr, mask, bg: CUDA tensors"""
    from osvos_pytorch_amd import _lib
    M, tone = np.ascontiguousarray(np.asarray(M, np.float64)), np.ascontiguousarray(np.asarray(tone, np.int32))
    n = M.shape[0] if n is None else n
    hh, ww = (int(v) for v in mask.shape)
    image = torch.full((max(n, 1), 3, hh, ww), float("nan"), device="cuda", dtype=torch.float32)
    gt = torch.full((max(n, 1), 1, hh, ww), float("nan"), device="cuda", dtype=torch.float32)
    need = int(_lib.lib().osvos_lucid_compose_ex_ws_bytes(max(min(n, 16), 1), hh, ww, max(min(band, 16), 0)))
    buf = torch.full((need + GUARD + 8,), GARBAGE_BYTE, device="cuda", dtype=torch.uint8)
    assert buf.data_ptr() % 8 == 0
    vp = C.c_void_p
    occ_a = None if occ is None else np.ascontiguousarray(np.asarray(occ, np.int32))
    d_t = None
    if D is not None:
        flat = np.zeros(np.asarray(D).size + 4, np.int16)
        flat[d_offset:d_offset + np.asarray(D).size] = np.asarray(D, np.int16).ravel()
        d_t = torch.from_numpy(flat).cuda()
        assert d_t.data_ptr() % 4 == 0
    wsp = None if ws is None else vp(buf.data_ptr() + ws_offset) if ws == "own" else vp(ws)
    rc = _lib.lib().osvos_lucid_compose_ex(vp(bgr.data_ptr()), vp(mask.data_ptr()), vp(bg.data_ptr()), vp(M.ctypes.data), vp(tone.ctypes.data),
                                           None if occ_a is None else vp(occ_a.ctypes.data), None if d_t is None else vp(d_t.data_ptr() + 2 * d_offset),
                                           cell, band, (C.c_float * 3)(*mean), vp(image.data_ptr()), vp(gt.data_ptr()), n, hh if h is None else h,
                                           ww if w is None else w, wsp, _stream())
    torch.cuda.synchronize()
    return rc, image, gt, buf, need


def _ex(bgr, mask, bg, M, tone, occ=None, D=None, cell=64, band=0, mean=lc.MEAN):
    from osvos_pytorch_amd import _lib
    rc, image, gt, buf, need = _ex_rc(bgr, mask, bg, M, tone, occ, D, cell, band, mean)
    _lib.check(rc, "lucid_compose_ex")
    n, (h, w) = len(M), mask.shape
    assert need == (8 * n * h * ((w + 63) // 64) if band else 0)
    assert bool((buf[need:] == GARBAGE_BYTE).all()), "the call wrote past osvos_lucid_compose_ex_ws_bytes"
    return image, gt


def _on_device(r):
    return _dev(r["bgr"]), _dev(r["mask"]), _dev(r["bg"])


def _against_restatement(c):
    r = ld.reference(c)
    image, gt = _ex(*_on_device(r), r["M"], r["tone"], r["occ"], r["D"], r["cell"], r["band"])
    print("%s: %d of %d image words and %d of %d labels differ; %d void" % (ld.case_id(c), int((_bits(image) != r["image"].view(np.uint32)).sum()),
                                                                            r["image"].size, int((_np(gt) != r["gt"]).sum()), r["gt"].size, int((r["gt"] < 0).sum())))
    assert np.array_equal(_bits(image), r["image"].view(np.uint32))
    assert np.array_equal(_bits(gt), r["gt"].view(np.uint32))


@pytest.mark.parametrize("c", ld.CASES, ids=ld.case_id)
def test_compose_ex_against_the_restatement(c):
    _against_restatement(c)


def test_compose_ex_on_a_davis_sized_frame():
    _against_restatement(ld.LARGE)


def test_the_cases_reach_what_they_are_there_for():
    """(no GPU work: the shared references)  void pixels on both sides of the word boundary; a band taller than the image; a covered
    frame; extreme fields push every tap out of the frame"""
    gt = ld.reference(ld.CASES[2])["gt"][0, 0]
    assert (gt[:, 63] == -1).all() and (gt[:, 64] == -1).all() and (gt[:, 62] == 1).all() and (gt[:, 65] == 0).all()
    gt = ld.reference(ld.CASES[3])["gt"][0, 0]                      # band 16 on five rows: every row of the disc but five falls outside
    assert (gt[:, 48:] == -1).all() and (gt[:, :48] == 1).all()
    assert (ld.reference(ld.CASES[5])["gt"] != 1).all() and (ld.reference(ld.CASES[5])["gt"] == -1).any()
    assert not ld.reference(ld.CASES[12])["gt"].any()
    assert not ld.reference(ld.CASES[14])["gt"].any() and not ld.reference(ld.CASES[15])["gt"].any()
    large = ld.reference(ld.LARGE)["gt"]
    assert (large == -1).any() and (large == 0).any() and (large == 1).any()


def test_samples_of_a_batch_are_independent_and_calls_repeat():
    c = ld.BATCH
    r = ld.reference(c)
    assert c[4] == 16
    dev = _on_device(r)
    image, gt = _ex(*dev, r["M"], r["tone"], r["occ"], r["D"], r["cell"], r["band"])
    again = _ex(*dev, r["M"], r["tone"], r["occ"], r["D"], r["cell"], r["band"])
    assert np.array_equal(_bits(image), _bits(again[0])) and np.array_equal(_bits(gt), _bits(again[1]))
    for i in (0, 7, 15):
        one = _ex(*dev, r["M"][i:i + 1], r["tone"][i:i + 1], r["occ"][i:i + 1], r["D"][i:i + 1], r["cell"], r["band"])
        assert np.array_equal(_bits(image[i:i + 1]), _bits(one[0])) and np.array_equal(_bits(gt[i:i + 1]), _bits(one[1])), i
    assert not torch.equal(gt[0], gt[1])


@pytest.mark.parametrize("c", [lc.COMPOSE_CASES[2], lc.COMPOSE_CASES[8], lc.COMPOSE_CASES[11]], ids=lc.case_id)
def test_everything_off_is_osvos_lucid_compose_bit_for_bit(c):
    from osvos_pytorch_amd import lucid
    r = lc.compose_reference(c)
    h, w, n = c[0], c[1], c[4]
    dev = _on_device(r)
    want = lucid.compose(*dev, r["M"], r["tone"])
    for kw in (dict(), dict(D=ld.field_of("zero", n, h, w, 8), cell=8), dict(occ=ld.occluders_of("rx0", n, h, w)), dict(cell=7),
               dict(D=ld.field_of("zero", n, h, w, 256), cell=256, occ=np.zeros((n, 6), np.int32))):
        image, gt = _ex(*dev, r["M"], r["tone"], **kw)
        assert np.array_equal(_bits(image), _bits(want[0])) and np.array_equal(_bits(gt), _bits(want[1])), kw.keys()
    assert np.array_equal(_bits(want[0]), r["image"].view(np.uint32))


def test_band_does_not_touch_the_image_and_only_voids_labels():
    c = ld.CASES[9]
    r = ld.reference(c)
    dev = _on_device(r)
    with_band = _ex(*dev, r["M"], r["tone"], r["occ"], r["D"], r["cell"], r["band"])
    without = _ex(*dev, r["M"], r["tone"], r["occ"], r["D"], r["cell"], 0)
    assert np.array_equal(_bits(with_band[0]), _bits(without[0]))
    void = with_band[1] < 0
    assert bool(void.any()) and torch.equal(with_band[1][~void], without[1][~void]) and bool((with_band[1][void] == -1).all())


def test_bad_arguments_return_an_error_and_launch_nothing():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    h, w = 12, 20
    bgr, mask, bg = _dev(lc.frame_of("noise", h, w, 1)), _dev(lc.mask_of("blob", h, w)), _dev(lc.frame_of("gradient", h, w))
    good_m, good_t = lc.params_of("rot30_s075", h, w, 2)
    good = dict(occ=ld.occluders_of("inside", 2, h, w), D=ld.field_of("smooth", 2, h, w, 8), cell=8, band=3)

    def refused(word, M=good_m, tone=good_t, **kw):
        rc, image, gt, buf, _ = _ex_rc(bgr, mask, bg, M, tone, **dict(good, **kw))
        assert rc < 0 and word in l.osvos_last_error(), (word, rc, l.osvos_last_error())
        assert bool(torch.isnan(image).all()) and bool(torch.isnan(gt).all()) and bool((buf == GARBAGE_BYTE).all()), word

    assert _ex_rc(bgr, mask, bg, good_m, good_t, **good)[0] == 0
    # what osvos_lucid_compose refuses
    refused(b"N", n=0)
    refused(b"N", M=good_m * 9, tone=good_t * 9, n=17, occ=None, D=None)
    refused(b"size", h=0)
    refused(b"size", w=4097)
    m = np.array(good_m, np.float64)
    m[1, 1, 2] = float("nan")
    refused(b"finite", M=m)
    m[1, 1, 2] = 2.0 ** 18 + 1
    refused(b"matrix", M=m)
    t = np.array(good_t, np.int32)
    t[1, 0, 1] = 1025
    refused(b"gain", tone=t)
    t = np.array(good_t, np.int32)
    t[0, 1, 4] = 256
    refused(b"offset", tone=t)
    # the lattice
    for cell in (0, 4, 7, 12, 24, 512, -8):
        refused(b"cell", cell=cell)
    assert _ex_rc(bgr, mask, bg, good_m, good_t, **dict(good, D=None, cell=7))[0] == 0      # without D the cell is not looked at
    refused(b"aligned", d_offset=1)
    # the band and its workspace
    refused(b"band", band=-1)
    refused(b"band", band=17)
    refused(b"null", ws=None)
    for off in (1, 2, 4):
        refused(b"aligned", ws_offset=off)
    refused(b"overlaps", ws=bgr.data_ptr() & ~7)
    assert _ex_rc(bgr, mask, bg, good_m, good_t, **dict(good, band=0, ws=None))[0] == 0     # band 0 needs none
    # the occluder
    for k, v in [(2, -1), (2, 4097), (3, -1), (3, 4097), (0, 8193), (0, -8193), (1, 8193), (4, -8193), (5, 8193), (5, -2 ** 31)]:
        occ = np.array(good["occ"], np.int64)
        occ[1, k] = v
        refused(b"radius" if k in (2, 3) else b"centre" if k < 2 else b"offset", occ=occ.astype(np.int32))
    occ = np.array([[8192, -8192, 4096, 4096, -8192, 8192]] * 2, np.int32)                   # the limits themselves are taken
    assert _ex_rc(bgr, mask, bg, good_m, good_t, **dict(good, occ=occ))[0] == 0
    # null pointers
    vp = C.c_void_p
    image = torch.full((1, 3, h, w), float("nan"), device="cuda")
    gt = torch.full((1, 1, h, w), float("nan"), device="cuda")
    m, t, mean = np.array(good_m, np.float64), np.array(good_t, np.int32), (C.c_float * 3)(*lc.MEAN)
    ptrs = [vp(bgr.data_ptr()), vp(mask.data_ptr()), vp(bg.data_ptr()), vp(m.ctypes.data), vp(t.ctypes.data), None, None, 64, 0, mean,
            vp(image.data_ptr()), vp(gt.data_ptr())]
    for i in (0, 1, 2, 3, 4, 9, 10, 11):
        a = list(ptrs)
        a[i] = None
        assert l.osvos_lucid_compose_ex(*a, 1, h, w, None, _stream()) < 0 and b"null" in l.osvos_last_error(), i
    torch.cuda.synchronize()
    assert bool(torch.isnan(image).all()) and bool(torch.isnan(gt).all())


def test_workspace_size_query():
    from osvos_pytorch_amd import _lib
    q = _lib.lib().osvos_lucid_compose_ex_ws_bytes
    assert q(1, 480, 854, 1) == 8 * 480 * 14 and q(3, 480, 854, 16) == 3 * 8 * 480 * 14 and q(16, 1, 1, 5) == 128
    assert q(1, 5, 64, 1) == 40 and q(1, 5, 65, 1) == 80 and q(16, 4096, 4096, 16) == 8 * 16 * 4096 * 64
    assert q(3, 480, 854, 0) == 0
    for bad in [(0, 8, 8, 1), (17, 8, 8, 1), (1, 0, 8, 1), (1, 8, 0, 1), (1, 4097, 8, 1), (1, 8, 4097, 1), (1, 8, 8, -1), (1, 8, 8, 17)]:
        assert q(*bad) == 0, bad


def test_wrappers_match_the_direct_calls():
    from osvos_pytorch_amd import lucid
    c = ld.CASES[9]
    r = ld.reference(c)
    h, w, n, cell, band = c[0], c[1], c[4], c[6], c[8]
    dev = _on_device(r)
    want = (r["image"].view(np.uint32), r["gt"].view(np.uint32))
    image, gt = lucid.compose(*dev, r["M"].tolist(), r["tone"].tolist(), occluders=r["occ"].tolist(), field=r["D"].tolist(), cell=cell, band=band)
    assert tuple(image.shape) == (n, 3, h, w) and tuple(gt.shape) == (n, 1, h, w) and image.dtype == gt.dtype == torch.float32
    assert np.array_equal(_bits(image), want[0]) and np.array_equal(_bits(gt), want[1])
    big = torch.full((1 << 12,), -1, device="cuda", dtype=torch.int64)
    image, gt = lucid.compose(*dev, r["M"], r["tone"], occluders=r["occ"], field=_dev(r["D"]), cell=cell, band=band, ws=big)      # a device field, a given ws
    assert np.array_equal(_bits(image), want[0]) and np.array_equal(_bits(gt), want[1]) and not bool((big == -1).all())
    small = torch.full((1,), -1, device="cuda", dtype=torch.int64)                                                           # too small: replaced, untouched
    assert np.array_equal(_bits(lucid.compose(*dev, r["M"], r["tone"], band=band, ws=small)[1]),
                          ld.compose_ex(r["bgr"], r["mask"], r["bg"], r["M"], r["tone"], band=band)[1].view(np.uint32)) and int(small[0]) == -1
    only = lucid.compose(*dev, r["M"], r["tone"], field=r["D"], cell=cell)
    assert np.array_equal(_bits(only[0]), ld.compose_ex(r["bgr"], r["mask"], r["bg"], r["M"], r["tone"], D=r["D"], cell=cell)[0].view(np.uint32))
    plain = lucid.compose(*dev, r["M"], r["tone"])                                                                            # called as before
    again = lucid.compose(*dev, r["M"], r["tone"], lc.MEAN, None, None, 64, 0, None)
    assert np.array_equal(_bits(plain[0]), _bits(again[0])) and torch.equal(plain[1], again[1])
    assert np.array_equal(_bits(plain[0]), lc.compose(r["bgr"], r["mask"], r["bg"], r["M"], r["tone"])[0].view(np.uint32))
    assert lucid.field_shape(h, w, cell) == tuple(r["D"].shape[1:3])
    bad_occ = r["occ"].copy()
    bad_occ[0, 2] = 4097
    for kw in [dict(band=17), dict(band=-1), dict(band=1.5), dict(occluders=bad_occ), dict(occluders=r["occ"][:1]), dict(occluders=r["occ"].astype(np.float32)),
               dict(field=r["D"], cell=cell // 2), dict(field=r["D"], cell=24), dict(field=r["D"][:1], cell=cell), dict(field=r["D"].astype(np.float32), cell=cell),
               dict(field=_dev(r["D"]).int(), cell=cell), dict(field=r["D"].astype(np.int32) + 40000, cell=cell)]:
        with pytest.raises(ValueError):
            lucid.compose(*dev, r["M"], r["tone"], **kw)


def test_lucid_dream_with_the_options():
    """LucidDream's draws with the options on, against lucid_deform_cases.draw on the same random stream: 13 numbers, then the field in the
    order (gy, gx, dx then dy), then the occluder's seven; batch(n) is one compose call over n of them and leaves random where n draws do"""
    from osvos_pytorch_amd import lucid
    r = lc.scenario_reference()
    s = lc.SCENE
    frame, mask = _dev(r["frame"]), _dev(r["mask"])
    kw = dict(deform=0.75, deform_cell=16, occlude=0.6, band=3)
    dream = lucid.LucidDream(frame, mask, meanval=(0.0, 0.0, 0.0), **dict(lc.DEFAULTS, **kw))
    plain = lucid.LucidDream(frame, mask, meanval=(0.0, 0.0, 0.0), **lc.DEFAULTS)
    gh, gw = ld.field_shape(s["h"], s["w"], 16)
    random.seed(11)
    draws = [dream.draw() for _ in range(3)]
    state = random.getstate()
    random.seed(11)
    for d in draws:                                                   # the restated order
        m, t = plain.draw()[:2]
        field, occ = ld.draw(random.random, dream.box, s["h"], s["w"], 0.75, 16, 0.6)
        assert d[0] == m and d[1] == t and np.array_equal(np.asarray(d[2]), field) and list(d[3]) == occ
        assert np.asarray(d[2]).shape == (gh, gw, 2)
    assert random.getstate() == state
    assert any(d[3][2] > 0 for d in draws) and any(np.asarray(d[2]).any() for d in draws)
    random.seed(11)
    got = dream.batch(3)
    assert random.getstate() == state
    want = ld.compose_ex(r["frame"], r["mask"], r["bg"], [d[0] for d in draws], [d[1] for d in draws], [d[3] for d in draws],
                         np.asarray([d[2] for d in draws], np.int16), 16, 3, (0.0, 0.0, 0.0))
    assert np.array_equal(_bits(got["image"]), want[0].view(np.uint32)) and np.array_equal(_bits(got["gt"]), want[1].view(np.uint32))
    assert (want[1] == -1).any() and (want[1] == 1).any() and (want[1] == 0).any()
    random.seed(11)
    one = dream()
    assert tuple(one["gt"].shape) == (1, s["h"], s["w"]) and np.array_equal(_bits(one["image"]), want[0][0].view(np.uint32))
    assert np.array_equal(_bits(one["gt"]), want[1][0].view(np.uint32))
    # each option alone draws only its own numbers; with all off, the 13 of before
    for kw, count in ((dict(), 13), (dict(band=16), 13), (dict(occlude=0.01), 20), (dict(deform=0.5, deform_cell=64), 13 + 2 * 2 * 2)):
        d = lucid.LucidDream(frame, mask, **kw)
        random.seed(3)
        d.batch(2)
        state = random.getstate()
        random.seed(3)
        for _ in range(2 * count):
            random.random()
        assert random.getstate() == state, kw
    # an empty mask: seven numbers all the same, no occluder
    empty = lucid.LucidDream(frame, torch.zeros_like(mask), occlude=1.0, band=2)
    random.seed(3)
    assert empty.draw()[3] == [0] * 6 and not bool(empty()["gt"].any())
    for bad in (dict(deform=1.5), dict(occlude=-1), dict(band=17), dict(deform_cell=24)):
        with pytest.raises(ValueError):
            lucid.LucidDream(frame, mask, **bad)


def _run_script(tmp, *args):
    return script_runner.train_online(tmp, "--device-augment", *args).stdout


def _png(tmp):
    with open(os.path.join(str(tmp), "Results", "blackswan", "00000.png"), "rb") as fh:
        return fh.read()


def _losses(out):
    return [float(line.split()[1]) for line in out.splitlines() if line.startswith("Loss: ")]


FULL = ("--lucid", "1", "--lucid-deform", "0.5,16", "--lucid-occlude", "0.5", "--lucid-band", "3")


def test_train_online_with_deformed_occluded_void_banded_samples(tmp_path):
    out = _run_script(tmp_path / "on", *FULL)
    losses = _losses(out)
    assert "Online training time" in out and "J&F on blackswan:" in out and losses and np.isfinite(losses).all(), out[-2000:]


def test_train_online_multi_object_with_the_options(tmp_path):
    out = _run_script(tmp_path / "on", "--multi-object", *FULL)
    assert "J&F on blackswan (2 objects):" in out and np.isfinite(_losses(out)).all() and len(_losses(out)) >= 2, out[-2000:]


def test_train_online_with_the_options_off_writes_the_same_bytes(tmp_path):
    _run_script(tmp_path / "off", "--lucid", "0.5", "--lucid-deform", "0", "--lucid-occlude", "0", "--lucid-band", "0")
    _run_script(tmp_path / "plain", "--lucid", "0.5")
    assert _png(tmp_path / "off") == _png(tmp_path / "plain")
