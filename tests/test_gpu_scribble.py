"""GPU: interactive scribbles on the device -- osvos_scribble_raster and osvos_mask_thin (csrc/scribble.hip) bit for bit against the
restatements of tests/scribble_cases.py, the two thinning paths against each other, the simulated annotator of osvos_pytorch_amd.scribble
against its numpy restatement, a session sample through the void-aware loss, and train_online.py --interactive.

The raster's LDS list holds OSVOS_SCRIBBLE_LIST_CAP = 512 rows and a cull chunk is 256 rows: the case "many" puts 700 segments over one
tile, which takes three chunks and two passes.  Outputs are pre-filled with garbage (7, a value neither kernel writes for these inputs)."""
import re

import numpy as np
import pytest
import torch

import scribble_cases as sc
import script_runner

pytestmark = pytest.mark.gpu
RASTER = sc.raster_cases()
THIN = sc.thin_cases()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- raster --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(RASTER))
def test_raster_equals_the_restatement_bit_for_bit(name):
    from osvos_pytorch_amd import scribble
    segs, (n, h, w) = RASTER[name]
    table = _cuda(segs)
    for r in sc.RADII:
        out = torch.full((n, h, w), 7, device="cuda", dtype=torch.uint8)
        got = scribble.raster_segments(table, (h, w), r, n, out=out)
        assert got is out
        want = sc.raster_ref(segs, n, h, w, r)
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg="%s radius %d" % (name, r))
        again = scribble.raster_segments(table, (h, w), r, n)          # no atomics: the same bytes every run
        assert torch.equal(again, got)
    if name == "none":
        assert (got == 255).all()


def test_raster_many_segments_take_more_than_one_chunk_and_pass():
    from osvos_pytorch_amd import _lib
    segs, _ = RASTER["many"]
    over_first_tile = ((segs[:, [0, 2]] < 64).all(axis=1) & (segs[:, [1, 3]] < 16).all(axis=1)).sum()
    assert over_first_tile == 700 > _lib.SCRIBBLE_LIST_CAP >= 512


def test_rasterize_from_host_paths_later_strokes_overrule_and_frames_stay_apart():
    from osvos_pytorch_amd import scribble
    paths = [(0, 1, [(2, 2), (60, 30), (69, 5)]), (1, 2, [(10, 10)]), (0, 0, [(60, 2), (2, 30)]), (2, 5, [(0, 39), (39, 0)]), (0, 3, [(30, 16)])]
    out = scribble.rasterize(paths, (40, 70), radius=2, frames=3)
    table = scribble.segment_table(paths, 3)
    assert table.shape == (6, 6)
    np.testing.assert_array_equal(out.cpu().numpy(), sc.raster_ref(table, 3, 40, 70, 2))
    o = out.cpu().numpy()
    assert o[0, 16, 30] == 3 and set(np.unique(o[1])) == {2, 255} and set(np.unique(o[2])) == {5, 255} and (o[1] == 2).sum() == 13
    empty = scribble.rasterize([], (40, 70), radius=64, frames=2)
    assert (empty == 255).all() and tuple(empty.shape) == (2, 40, 70)


# ---- thinning ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_iters", [64, 1, 2])
@pytest.mark.parametrize("name", list(THIN))
def test_thin_both_paths_equal_the_restatement_with_info(name, max_iters):
    from osvos_pytorch_amd import scribble
    mask = THIN[name]
    want, winfo = sc.thin_ref(mask, max_iters)
    got = {}
    for path in (1, 2):
        out = torch.full(mask.shape, 7, device="cuda", dtype=torch.uint8)
        skel, info = scribble.thin(_cuda(mask), max_iters, path, out=out)
        assert skel is out and info.dtype == torch.int32
        np.testing.assert_array_equal(skel.cpu().numpy(), want, err_msg="%s path %d" % (name, path))
        np.testing.assert_array_equal(info.cpu().numpy(), winfo, err_msg="%s path %d info" % (name, path))
        got[path] = skel
    assert torch.equal(got[1], got[2])
    if max_iters == 64:
        for n in range(mask.shape[0]):
            assert sc.count8(want[n]) == sc.count8(mask[n])
    if name == "square40" and max_iters < 64:
        assert winfo.tolist() == [[max_iters, 0]]


def test_thin_takes_bool_masks_writes_in_place_and_is_idempotent():
    from osvos_pytorch_amd import scribble
    mask = THIN["blobs"]
    want, _ = sc.thin_ref(mask)
    for path in (0, 1, 2):
        m = _cuda(mask != 0)
        skel, info = scribble.thin(m, path=path)
        np.testing.assert_array_equal(skel.cpu().numpy(), want)
        buf = _cuda(mask).clone()
        same, _ = scribble.thin(buf, path=path, out=buf)          # out may be the mask
        assert same is buf and torch.equal(buf, skel)
        again, info2 = scribble.thin(skel, path=path)
        assert torch.equal(again, skel) and info2.cpu().tolist() == [[1, 1]] * mask.shape[0]


def test_thin_a_plane_too_large_for_lds_goes_the_global_path():
    from osvos_pytorch_amd import _lib, scribble
    mask = sc.wide_case()
    n, h, w = mask.shape
    assert h * ((w + 63) // 64) > _lib.THIN_RESIDENT_WORDS
    want, winfo = sc.thin_ref(mask)
    m = _cuda(mask)
    skel, info = scribble.thin(m, path=0)
    np.testing.assert_array_equal(skel.cpu().numpy(), want)
    np.testing.assert_array_equal(info.cpu().numpy(), winfo)
    assert len(set(winfo[:, 0].tolist())) > 1                      # frames that stop after different numbers of iterations
    with pytest.raises(ValueError, match="path 1 keeps the 1-bit plane in LDS"):
        scribble.thin(m, path=1)
    info = torch.zeros((n, 2), device="cuda", dtype=torch.int32)
    ws = torch.empty(_lib.lib().osvos_mask_thin_ws_bytes(n, h, w), device="cuda", dtype=torch.uint8)
    rc = _lib.lib().osvos_mask_thin(m.data_ptr(), skel.data_ptr(), info.data_ptr(), n, h, w, 64, 1, ws.data_ptr(), None)
    assert rc < 0 and b"path 1" in _lib.lib().osvos_last_error()


# ---- the simulated annotator -----------------------------------------------------------------------------------------------------------------

def _annotator_problem():
    gt = np.stack([sc.blob(48, 64, 11, 0.3), sc.blob(48, 64, 12, 0.4)]).astype(np.uint8)
    pred = np.stack([sc.blob(48, 64, 13, 0.3), sc.blob(48, 64, 12, 0.4)]).astype(np.uint8)
    pred[1, 5:20, 5:25] ^= 1
    pred[1, 40, 60] ^= 1
    return pred, gt


def test_initial_and_error_scribbles_equal_the_numpy_restatement():
    from osvos_pytorch_amd import scribble
    pred, gt = _annotator_problem()
    first = scribble.initial_scribbles(_cuda(gt), radius=3).cpu().numpy()
    np.testing.assert_array_equal(first, sc.initial_ref(gt, 3))
    assert all((first[n] == 1).any() and (first[n] == 0).any() for n in range(2))          # the first interaction carries both classes
    err = pred != gt
    for min_area, keep_largest in ((16, False), (64, True), (0, False)):
        out = scribble.error_scribbles(_cuda(pred), _cuda(gt), min_area, keep_largest, radius=2).cpu().numpy()
        np.testing.assert_array_equal(out, sc.error_ref(pred, gt, min_area, keep_largest, 2), err_msg=str((min_area, keep_largest)))
        assert not ((out != 255) & ~err).any()                                                   # no labelled pixel outside E
        assert ((out == gt) | (out == 255)).all()                                                # a stroke carries the true label
        if not keep_largest:
            for n in range(2):
                lab = sc.components8(err[n])
                for i in np.unique(lab[lab > 0]):
                    assert ((out[n] != 255) & (lab == i)).any() == ((lab == i).sum() >= min_area)   # every region of min_area pixels gets a stroke
    robot = scribble.Robot(radius=2, min_area=16, keep_largest=False)
    np.testing.assert_array_equal(robot(_cuda(pred[1]), _cuda(gt[1])).cpu().numpy(), sc.error_ref(pred[1:], gt[1:], 16, False, 2)[0])
    np.testing.assert_array_equal(robot(None, _cuda(gt[0])).cpu().numpy(), sc.initial_ref(gt[:1], 2)[0])


def test_training_planes_and_the_prior():
    from osvos_pytorch_amd import scribble
    m = np.full((20, 30), 255, dtype=np.uint8)
    m[2, 2:10] = 1
    m[15, 20:28] = 0
    prev = np.zeros((20, 30), dtype=np.uint8)
    prev[:, :15] = 1
    lab, obj = (t.cpu().numpy() for t in scribble.training_planes(_cuda(m), 1))
    np.testing.assert_array_equal(lab, np.where(m != 255, 255, 0))
    np.testing.assert_array_equal(obj, np.where(m == 1, 255, 0))
    lab, obj = (t.cpu().numpy() for t in scribble.training_planes(_cuda(m), 1, _cuda(prev), prior_distance=4))
    far = sc.sqdist_to(m != 255) > 16
    np.testing.assert_array_equal(lab != 0, (m != 255) | far)
    np.testing.assert_array_equal(obj != 0, (m == 1) | (far & (prev != 0)))


def test_a_session_sample_through_the_loss_has_gradient_zero_on_void_pixels():
    from osvos_pytorch_amd.layers.osvos_layers import class_balanced_cross_entropy_loss_step
    from osvos_pytorch_amd import scribble
    from osvos_pytorch_amd.augment import DeviceAugment
    import random
    random.seed(3)
    _, gt = _annotator_problem()
    rng = np.random.RandomState(2)
    frame = _cuda(rng.randint(0, 256, size=(48, 64, 3)).astype(np.uint8))
    session = scribble.InteractiveSession(None, None, [frame], object_id=1, augment=DeviceAugment(rots=(-30, 30), scales=(.75, 1.25)), loop=object())
    assert session.add(0, scribble.initial_scribbles(_cuda(gt[:1]))[0]) is True
    image, label = session.sample(0)
    assert tuple(image.shape) == (1, 3, 48, 64) and tuple(label.shape) == (1, 1, 48, 64)
    values = set(np.unique(label.cpu().numpy()).tolist())
    assert values == {-1.0, 0.0, 1.0}
    logits = _cuda(rng.randn(1, 1, 48, 64).astype(np.float32))
    loss, grad = class_balanced_cross_entropy_loss_step(logits, label, size_average=False, void_labels=True)
    g, lab = grad.cpu().numpy(), label.cpu().numpy()
    assert np.isfinite(float(loss)) and float(loss) > 0
    assert (g[lab < 0] == 0).all()                       # exactly 0 wherever the label is -1
    assert (g[lab == 1] != 0).any() and (g[lab == 0] != 0).any()
    # a sample with one class contributes exactly nothing: the rule that keeps such frames out of the rotation
    one = torch.where(label == 0, torch.full_like(label, -1.0), label)
    loss1, grad1 = class_balanced_cross_entropy_loss_step(logits, one, size_average=False, void_labels=True)
    assert float(loss1) == 0.0 and (grad1 == 0).all()


# ---- the script -----------------------------------------------------------------------------------------------------------------------------

def test_train_online_interactive(tmp_path):
    r = script_runner.train_online(tmp_path, "--device-augment", "--synthetic-frames", "3", "--interactive", "2,3,2", frames=3)
    rounds = re.findall(r"^Interactive round (\d+) on blackswan: frame (\S+) annotated, (\d+) labelled pixels, J ([0-9.]+) F ([0-9.]+), "
                        r"fit ([0-9.]+) s, predict ([0-9.]+) s$", r.stdout, re.M)
    assert [int(m[0]) for m in rounds] == [0, 1] and rounds[0][1] == "0", r.stdout[-2000:]
    assert 0 < int(rounds[0][2]) <= int(rounds[1][2])
    final = re.search(r"^Interactive J&F on blackswan per round: ([0-9.]+) ([0-9.]+) mean ([0-9.]+)$", r.stdout, re.M)
    assert final, r.stdout[-2000:]
    jf = [0.5 * (float(m[3]) + float(m[4])) for m in rounds]
    assert abs(float(final.group(1)) - jf[0]) < 2e-4 and abs(float(final.group(2)) - jf[1]) < 2e-4
    assert abs(float(final.group(3)) - 0.5 * (jf[0] + jf[1])) < 2e-4
    assert len(r.masks) == 3 and all(m[:8] == b"\x89PNG\r\n\x1a\n" for m in r.masks)
