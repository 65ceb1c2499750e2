"""GPU: superpixel snapping on the device -- osvos_superpixels_slic and osvos_superpixels_pool (csrc/superpixels.hip) against the numpy
restatement of the rule in tests/superpixel_cases.py, bit for bit (the rule is integer arithmetic: every comparison is np.array_equal, there
is no tolerance), their exact properties, the wrappers of osvos_pytorch_amd.superpixels, the snapping scenario through SuperpixelSnapper,
and train_online.py --snap-cell.  labels, centres, out and both workspaces are pre-filled with garbage before every call."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import superpixel_cases as sc
import script_runner

pytestmark = pytest.mark.gpu
GARBAGE_INT = 0x5a5a5a5a
GARBAGE_BYTE = 0xa5
GUARD = 256


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _garbage_ws(need):
    """a garbage-filled workspace of exactly `need` bytes inside a larger buffer: (the whole buffer, the size asked for)"""
    return torch.full((need + GUARD,), GARBAGE_BYTE, device="cuda", dtype=torch.uint8), need


def _slic_ws(n, h, w, cell):
    from osvos_pytorch_amd import _lib
    need = int(_lib.lib().osvos_superpixels_ws_bytes(n, h, w, cell))
    assert need >= n * int(np.prod(sc.grid_shape(h, w, cell))) * 6 * 4
    return _garbage_ws(need)


def _pool_ws(n, k):
    from osvos_pytorch_amd import _lib
    need = int(_lib.lib().osvos_superpixels_pool_ws_bytes(n, k))
    assert need >= n * k * 12
    return _garbage_ws(need)


def _slic_rc(frames, cell, m, iters, with_centres=True, ws=None):
    """one osvos_superpixels_slic call through _lib on a CUDA uint8 [N,H,W,3] tensor -> (rc, labels, centres or None, ws buffer, ws bytes)"""
    from osvos_pytorch_amd import _lib
    n, h, w = (int(v) for v in frames.shape[:3])
    gh, gw = sc.grid_shape(h, w, min(max(cell, 2), 64))
    labels = torch.full((n, h, w), GARBAGE_INT, device="cuda", dtype=torch.int32)
    centres = torch.full((n, gh * gw, 6), GARBAGE_INT, device="cuda", dtype=torch.int32) if with_centres else None
    buf, need = ws if ws is not None else _slic_ws(n, h, w, cell)
    vp = C.c_void_p
    rc = _lib.lib().osvos_superpixels_slic(vp(frames.data_ptr()), vp(labels.data_ptr()), vp(centres.data_ptr()) if with_centres else None,
                                           vp(buf.data_ptr()), n, h, w, cell, m, iters, _stream())
    return rc, labels, centres, buf, need


def _slic(frames, cell, m, iters, with_centres=True):
    from osvos_pytorch_amd import _lib
    rc, labels, centres, buf, need = _slic_rc(frames, cell, m, iters, with_centres)
    _lib.check(rc, "superpixels_slic")
    assert bool((buf[need:] == GARBAGE_BYTE).all()), "the call wrote past osvos_superpixels_ws_bytes"
    return labels, centres


def _pool_rc(logits, labels, k, ws=None, out=None):
    from osvos_pytorch_amd import _lib
    n, h, w = (int(v) for v in logits.shape)
    if out is None:
        out = torch.full_like(logits, float("nan"))
    buf, need = ws if ws is not None else _pool_ws(n, k)
    vp = C.c_void_p
    rc = _lib.lib().osvos_superpixels_pool(vp(logits.data_ptr()), vp(labels.data_ptr()), vp(out.data_ptr()), vp(buf.data_ptr()), n, h, w, k, _stream())
    return rc, out, buf, need


def _pool(logits, labels, k):
    from osvos_pytorch_amd import _lib
    rc, out, buf, need = _pool_rc(logits, labels, k)
    _lib.check(rc, "superpixels_pool")
    assert bool((buf[need:] == GARBAGE_BYTE).all()), "the call wrote past osvos_superpixels_pool_ws_bytes"
    return out


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                       # (a copy: the shared references are read-only)


def _np(t):
    return t.cpu().numpy()


def _bits(t):
    return _np(t).view(np.uint32)


def _against_restatement(kind, c):
    h, w, n, cell, m, iters = c
    r = sc.reference(kind, c)
    labels, centres = _slic(_dev(r["frames"]), cell, m, iters)
    labels, centres = _np(labels), _np(centres)
    print("%s %s: %d of %d labels and %d of %d clusters differ" % (sc.case_id(c), kind, int((labels != r["labels"]).sum()), labels.size,
                                                                  int((centres != r["centres"]).any(-1).sum()), centres.shape[0] * centres.shape[1]))
    assert np.array_equal(labels, r["labels"])
    assert np.array_equal(centres, r["centres"])


@pytest.mark.parametrize("kind", sc.SCENES)
@pytest.mark.parametrize("c", sc.SLIC_CASES, ids=sc.case_id)
def test_slic_against_the_restatement(c, kind):
    _against_restatement(kind, c)


@pytest.mark.parametrize("kind", sc.LARGE_SCENES)
def test_slic_on_a_davis_sized_frame(kind):
    _against_restatement(kind, sc.LARGE_CASE)


def _pool_check(logits, labels, k):
    out = _pool(_dev(logits), _dev(labels), k)
    want = sc.pool(logits, labels, k)
    print("pool %s K %d: %d of %d words differ" % (logits.shape, k, int((_bits(out) != want.view(np.uint32)).sum()), want.size))
    assert np.array_equal(_bits(out), want.view(np.uint32))


@pytest.mark.parametrize("c", [sc.SLIC_CASES[2], sc.SLIC_CASES[3], sc.SLIC_CASES[5]], ids=sc.case_id)
def test_pool_over_slic_labels(c):
    h, w, n, cell, m, iters = c
    r = sc.reference("noise", c)
    _pool_check(sc.awkward_logits((n, h, w), 1), r["labels"], r["centres"].shape[1])


@pytest.mark.parametrize("h,w,n,k", [(37, 53, 2, 11), (16, 300, 1, 4800), (45, 70, 1, 100000), (1, 1, 1, 1), (33, 65, 2, 1)])
def test_pool_over_arbitrary_labels(h, w, n, k):
    """uniformly random labels in [0, K): few labels (every pixel of a tile in the LDS table), more labels than the table holds, K far beyond
    the pixel count; and K = 1"""
    rng = np.random.default_rng([h, w, n, k])
    labels = rng.integers(0, k, size=(n, h, w)).astype(np.int32)
    _pool_check(sc.awkward_logits((n, h, w), 2), labels, k)


def test_pool_passes_labels_out_of_range_through():
    h, w, n, k = 37, 70, 2, 50
    rng = np.random.default_rng(3)
    labels = rng.integers(0, k, size=(n, h, w)).astype(np.int32)
    flat = labels.reshape(-1)
    flat[rng.permutation(flat.size)[:600]] = np.resize(np.array([-1, k, k + 1, -2 ** 31, 2 ** 31 - 1], np.int64), 600).astype(np.int32)
    logits = sc.awkward_logits((n, h, w), 3)
    _pool_check(logits, labels, k)
    # a frame where every label is out of range: the logits themselves
    out = _pool(_dev(logits), _dev(np.full_like(labels, k)), k)
    assert np.array_equal(_bits(out), logits.view(np.uint32))


def test_pool_on_a_davis_sized_frame():
    r = sc.reference("noise", sc.LARGE_CASE)
    rng = np.random.default_rng(4)
    logits = (rng.standard_normal((1, 480, 854)) * 5).astype(np.float32)
    _pool_check(logits, r["labels"], r["centres"].shape[1])


def test_frames_of_a_batch_are_independent_and_calls_repeat():
    c = (37, 53, 3, 8, 10, 4)
    h, w, n, cell, m, iters = c
    frames = _dev(sc.frames_of("noise", h, w, n))
    labels, centres = _slic(frames, cell, m, iters)
    again = _slic(frames, cell, m, iters)
    assert torch.equal(labels, again[0]) and torch.equal(centres, again[1])
    for i in range(n):
        one = _slic(frames[i:i + 1].contiguous(), cell, m, iters)
        assert torch.equal(labels[i:i + 1], one[0]) and torch.equal(centres[i:i + 1], one[1]), i
    assert not torch.equal(labels[0], labels[1])
    k = centres.shape[1]
    logits = _dev(sc.awkward_logits((n, h, w), 5))
    out = _pool(logits, labels, k)
    assert np.array_equal(_bits(out), _bits(_pool(logits, labels, k)))
    for i in range(n):
        assert np.array_equal(_bits(out[i:i + 1]), _bits(_pool(logits[i:i + 1].contiguous(), labels[i:i + 1].contiguous(), k))), i


def test_centres_may_be_null():
    c = sc.SLIC_CASES[2]
    r = sc.reference("gradient", c)
    labels, centres = _slic(_dev(r["frames"]), *c[3:], with_centres=False)
    assert centres is None and np.array_equal(_np(labels), r["labels"])


def test_workspace_size_queries():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    assert l.osvos_superpixels_ws_bytes(1, 480, 854, 8) >= 60 * 107 * 6 * 4
    assert l.osvos_superpixels_ws_bytes(2, 480, 854, 8) == 2 * l.osvos_superpixels_ws_bytes(1, 480, 854, 8)
    for bad in [(0, 8, 8, 8), (65536, 8, 8, 8), (1, 0, 8, 8), (1, 8, 16385, 8), (1, 8, 8, 1), (1, 8, 8, 65), (1, 8, 8, 0), (1, 8, 8, -2)]:
        assert l.osvos_superpixels_ws_bytes(*bad) == 0, bad
    assert l.osvos_superpixels_pool_ws_bytes(1, 6420) >= 6420 * 12
    for bad in [(0, 5), (65536, 5), (1, 0), (1, -1), (1, 2 ** 28 + 1)]:
        assert l.osvos_superpixels_pool_ws_bytes(*bad) == 0, bad


def test_bad_arguments_return_an_error_and_launch_nothing():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    h, w = 12, 20
    frames = _dev(sc.frames_of("noise", h, w, 1))
    for bad, word in [((1, 10, 5), b"cell"), ((65, 10, 5), b"cell"), ((0, 10, 5), b"cell"), ((8, -1, 5), b"compactness"), ((8, 65, 5), b"compactness"),
                      ((8, 10, -1), b"iters"), ((8, 10, 17), b"iters")]:
        rc, labels, centres, buf, _ = _slic_rc(frames, *bad, ws=_slic_ws(1, h, w, 8))
        assert rc < 0 and word in l.osvos_last_error(), (bad, l.osvos_last_error())
        torch.cuda.synchronize()
        assert bool((labels == GARBAGE_INT).all()) and bool((centres == GARBAGE_INT).all()) and bool((buf == GARBAGE_BYTE).all()), bad
    vp = C.c_void_p
    labels = torch.full((1, h, w), GARBAGE_INT, device="cuda", dtype=torch.int32)
    buf, _ = _slic_ws(1, h, w, 8)
    fp, lp, bp = vp(frames.data_ptr()), vp(labels.data_ptr()), vp(buf.data_ptr())
    tail = (8, 10, 5, _stream())
    assert l.osvos_superpixels_slic(None, lp, None, bp, 1, h, w, *tail) < 0 and b"null" in l.osvos_last_error()
    assert l.osvos_superpixels_slic(fp, None, None, bp, 1, h, w, *tail) < 0 and b"null" in l.osvos_last_error()
    assert l.osvos_superpixels_slic(fp, lp, None, None, 1, h, w, *tail) < 0 and b"null" in l.osvos_last_error()
    assert l.osvos_superpixels_slic(fp, lp, None, bp, 0, h, w, *tail) < 0 and b"N" in l.osvos_last_error()
    assert l.osvos_superpixels_slic(fp, lp, None, bp, 1, 0, w, *tail) < 0 and b"size" in l.osvos_last_error()
    assert l.osvos_superpixels_slic(fp, lp, None, bp, 1, h, 16385, *tail) < 0 and b"size" in l.osvos_last_error()
    assert l.osvos_superpixels_slic(fp, lp, None, lp, 1, h, w, *tail) < 0 and b"aliasing" in l.osvos_last_error()
    assert l.osvos_superpixels_slic(fp, lp, lp, bp, 1, h, w, *tail) < 0 and b"centres" in l.osvos_last_error()
    assert l.osvos_superpixels_slic(fp, lp, bp, bp, 1, h, w, *tail) < 0 and b"centres" in l.osvos_last_error()
    assert l.osvos_superpixels_slic(fp, vp(labels.data_ptr() + 2), None, bp, 1, h, w - 1, *tail) < 0 and b"aligned" in l.osvos_last_error()
    torch.cuda.synchronize()
    assert bool((labels == GARBAGE_INT).all()) and bool((buf == GARBAGE_BYTE).all())
    with pytest.raises(RuntimeError):
        _lib.check(-1, "superpixels_slic")
    # the pooling
    logits = _dev(sc.awkward_logits((1, h, w), 6))
    lab = torch.zeros((1, h, w), device="cuda", dtype=torch.int32)
    before = _bits(logits).copy()
    for k, word in [(0, b"K"), (-1, b"K"), (2 ** 28 + 1, b"K")]:
        rc, out, buf, _ = _pool_rc(logits, lab, k, ws=_pool_ws(1, 4))
        assert rc < 0 and word in l.osvos_last_error(), (k, l.osvos_last_error())
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and bool((buf == GARBAGE_BYTE).all())
    rc, _, buf, _ = _pool_rc(logits, lab, 4, out=logits)
    assert rc < 0 and b"out" in l.osvos_last_error()
    rc, _, _, _ = _pool_rc(logits, lab, 4, out=lab)
    assert rc < 0 and b"out" in l.osvos_last_error()
    out = torch.full_like(logits, float("nan"))
    xp, lp, op, bp = vp(logits.data_ptr()), vp(lab.data_ptr()), vp(out.data_ptr()), vp(buf.data_ptr())
    assert l.osvos_superpixels_pool(xp, lp, op, op, 1, h, w, 4, _stream()) < 0 and b"ws" in l.osvos_last_error()
    assert l.osvos_superpixels_pool(None, lp, op, bp, 1, h, w, 4, _stream()) < 0 and b"null" in l.osvos_last_error()
    assert l.osvos_superpixels_pool(xp, None, op, bp, 1, h, w, 4, _stream()) < 0
    assert l.osvos_superpixels_pool(xp, lp, None, bp, 1, h, w, 4, _stream()) < 0
    assert l.osvos_superpixels_pool(xp, lp, op, None, 1, h, w, 4, _stream()) < 0
    assert l.osvos_superpixels_pool(xp, lp, op, bp, 0, h, w, 4, _stream()) < 0 and b"N" in l.osvos_last_error()
    assert l.osvos_superpixels_pool(xp, lp, op, bp, 1, h, 0, 4, _stream()) < 0 and b"size" in l.osvos_last_error()
    assert l.osvos_superpixels_pool(xp, lp, op, vp(buf.data_ptr() + 4), 1, h, w, 4, _stream()) < 0 and b"aligned" in l.osvos_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool((buf == GARBAGE_BYTE).all()) and np.array_equal(_bits(logits), before) and not bool(lab.any())


def test_wrappers_match_the_direct_calls():
    from osvos_pytorch_amd import superpixels
    c = sc.SLIC_CASES[2]
    h, w, n, cell, m, iters = c
    r = sc.reference("noise", c)
    frames = _dev(r["frames"])
    k = r["centres"].shape[1]
    labels, centres = superpixels.slic(frames, cell, m, iters, with_centres=True)
    assert labels.dtype == torch.int32 and centres.dtype == torch.int32 and tuple(labels.shape) == (n, h, w) and tuple(centres.shape) == (n, k, 6)
    assert np.array_equal(_np(labels), r["labels"]) and np.array_equal(_np(centres), r["centres"])
    only = superpixels.slic(frames, cell=cell, compactness=m, iters=iters)
    assert torch.is_tensor(only) and torch.equal(only, labels)
    one = superpixels.slic(frames[0], cell, m, iters)                                        # [H,W,3] for one frame
    assert tuple(one.shape) == (1, h, w) and torch.equal(one[0], labels[0])
    big = torch.empty(1 << 20, device="cuda", dtype=torch.uint8)
    assert torch.equal(superpixels.slic(frames, cell, m, iters, ws=big), labels)
    x = sc.awkward_logits((n, h, w), 7)
    want = sc.pool(x, r["labels"], k).view(np.uint32)
    for shaped in (_dev(x), _dev(x)[:, None]):
        out = superpixels.pool(shaped, labels, k)
        assert out.shape == shaped.shape and out.dtype == torch.float32 and np.array_equal(_bits(out).reshape(want.shape), want)
    out = superpixels.pool(_dev(x)[0], labels[0], k, ws=big)                                  # [H,W] with [H,W] labels
    assert tuple(out.shape) == (h, w) and np.array_equal(_bits(out), want[0])
    out = superpixels.pool(_dev(x), labels)                                                   # k from the labels (one read-back)
    assert np.array_equal(_bits(out), sc.pool(x, r["labels"], int(r["labels"].max()) + 1).view(np.uint32))
    with pytest.raises(ValueError):
        superpixels.slic(frames.float(), cell, m, iters)
    with pytest.raises(ValueError):
        superpixels.slic(frames, cell=65)
    with pytest.raises(ValueError):
        superpixels.pool(_dev(x), labels[:, :-1], k)
    with pytest.raises(ValueError):
        superpixels.pool(_dev(x), labels.long(), k)
    with pytest.raises(ValueError):
        superpixels.pool(_dev(x).double(), labels, k)
    with pytest.raises(ValueError):
        superpixels.pool(_dev(x), labels, 0)


def test_snapper_with_labels_equals_the_version_without():
    from osvos_pytorch_amd import superpixels
    h, w, n = 45, 70, 3
    frames = _dev(sc.frames_of("gradient", h, w, n))
    snapper = superpixels.SuperpixelSnapper(cell=5, compactness=4, iters=2)
    labels = snapper.labels(frames)
    want_labels, _ = sc.slic(_np(frames), 5, 4, 2)
    assert np.array_equal(_np(labels), want_labels)
    k = int(np.prod(sc.grid_shape(h, w, 5)))
    for seed in (8, 9):                                                                       # two objects over the same frames
        x = sc.awkward_logits((n, 1, h, w), seed)
        a, b = snapper(_dev(x), frames), snapper(_dev(x), labels=labels)
        assert a.shape == (n, 1, h, w) and np.array_equal(_bits(a), _bits(b))
        assert np.array_equal(_bits(a)[:, 0], sc.pool(x[:, 0], want_labels, k).view(np.uint32))
    with pytest.raises(ValueError):
        snapper(_dev(x), frames, labels=labels)
    with pytest.raises(ValueError):
        snapper(_dev(x))


def test_snapping_scenario_on_the_device():
    """tests/test_superpixels_cpu.py pins the scenario on the restatement (IoU 0.8158 -> 1.0000, no impure superpixel); here the product
    runs it and gives the restatement's bytes, hence its IoUs"""
    from osvos_pytorch_amd import superpixels
    r = sc.snapping_reference()
    s = sc.SNAP
    snapper = superpixels.SuperpixelSnapper(s["cell"], s["compactness"], s["iters"])
    logits = _dev(r["logits"])
    out = snapper(logits, _dev(r["frame"]))
    assert tuple(out.shape) == (s["h"], s["w"])
    assert np.array_equal(_np(snapper.labels(_dev(r["frame"]))[0]), r["labels"])
    assert np.array_equal(_bits(out), r["pooled"].view(np.uint32))
    plain, pooled = sc.iou(_np(logits) > 0, r["truth"]), sc.iou(_np(out) > 0, r["truth"])
    print("snapping scenario on the device: IoU %.4f -> %.4f" % (plain, pooled))
    assert plain == r["iou_plain"] <= 0.90 and pooled == r["iou_pooled"] >= 0.99


def _run_script(tmp, *args):
    return script_runner.train_online(tmp, *args).stdout


def _train_online(tmp, *extra):
    r = script_runner.train_online(tmp, "--device-augment", "--synthetic-frames", "3", *extra, frames=3)
    return r.stdout, r.masks


def test_train_online_with_snapping(tmp_path):
    """the option on; and --snap-cell 0 against the command without the option, byte for byte.  (The two compared commands run without
    --track-components for the reason tests/test_gpu_flow.py gives: with the tracker two runs of the SAME plain command wrote different
    masks, because an untrained network's logits sit at the threshold; without it the written bytes repeat.)"""
    out, _ = _train_online(tmp_path / "on", "--snap-cell", "6")
    assert "Online training time" in out and "J&F on blackswan:" in out, out[-2000:]
    _, off = _train_online(tmp_path / "off", "--snap-cell", "0")
    _, plain = _train_online(tmp_path / "plain")
    assert off == plain


def test_train_online_multi_object_with_snapping(tmp_path):
    """the superpixels of the frames computed once and every object's logit stack pooled over them before the merge"""
    out = _run_script(tmp_path / "on", "--multi-object", "--snap-cell", "6", "--snap-iters", "2")
    assert "J&F on blackswan (2 objects):" in out and "J&F on blackswan object 2:" in out, out[-2000:]
    assert os.path.exists(os.path.join(str(tmp_path / "on"), "Results", "blackswan", "00000.png"))
