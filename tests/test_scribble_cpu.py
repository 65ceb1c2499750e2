"""CPU: the restatements the GPU tests of interactive scribbles compare against (tests/scribble_cases.py) hold the properties they must; the
Python layer of osvos_pytorch_amd.scribble reads the DAVIS layout, checks its arguments and refuses CPU tensors; the library refuses bad
arguments before any launch; train_online.py refuses the combinations the interactive loop does not run; and the session and the loop make
their calls in the stated order (recording stand-ins, as tests/test_sequence_cpu.py does it)."""
import ctypes as C
import io
import json
import os

import numpy as np
import pytest
import torch

import scribble_cases as sc


# ---- the restatements ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in sc.raster_cases() if n != "many"])
def test_raster_restatement_equals_the_brute_force_with_python_integers(name):
    segs, (n, h, w) = sc.raster_cases()[name]
    for r in sc.RADII:
        np.testing.assert_array_equal(sc.raster_ref(segs, n, h, w, r), sc.raster_bruteforce(segs, n, h, w, r), err_msg="%s radius %d" % (name, r))


def test_raster_restatement_on_700_segments_over_one_tile():
    segs, _ = sc.raster_cases()["many"]
    assert len(segs) == 700 > sc.LIST_CAP > 2 * sc.CHUNK - 1
    np.testing.assert_array_equal(sc.raster_ref(segs, 1, 16, 64, 1), sc.raster_bruteforce(segs, 1, 16, 64, 1))


def test_the_highest_index_wins_and_unlabelled_is_255():
    cases = sc.raster_cases()
    ab = sc.raster_ref(cases["overlap_ab"][0], 1, 33, 70, 3)
    ba = sc.raster_ref(cases["overlap_ba"][0], 1, 33, 70, 3)
    both = (ab != 255) & (ab != ba)          # where the two strokes cross
    assert both.any() and (ab[both] == 2).all() and (ba[both] == 1).all()
    np.testing.assert_array_equal(ab != 255, ba != 255)
    assert (sc.raster_ref(cases["none"][0], 1, 33, 70, 64) == 255).all()
    point = sc.raster_ref(cases["point"][0], 1, 33, 70, 0)
    assert (point == 3).sum() == 1 and point[0, 17, 40] == 3          # a degenerate segment of radius 0 is its one pixel
    frames = sc.raster_ref(cases["frames"][0], 3, 40, 40, 1)
    assert all((frames[f] != 255).any() for f in range(3))


@pytest.mark.parametrize("name", list(sc.thin_cases()))
def test_thinning_restatement_subset_idempotent_and_component_count(name):
    mask = sc.thin_cases()[name]
    skel, info = sc.thin_ref(mask, 64)
    assert set(np.unique(skel)) <= {0, 1}
    assert not (skel.astype(bool) & ~(mask != 0)).any()
    assert (info[:, 1] == 1).all() and (info[:, 0] <= 30).all(), info
    again, info2 = sc.thin_ref(skel, 64)
    np.testing.assert_array_equal(again, skel)
    assert (info2 == (1, 1)).all()
    for n in range(mask.shape[0]):
        assert sc.count8(skel[n]) == sc.count8(mask[n]), (name, n)


def test_thinning_small_shapes_and_info_when_max_iters_cuts_the_run_short():
    skel, info = sc.thin_ref(sc.thin_cases()["square2"], 64)
    assert skel.sum() == 1 and info.tolist() == [[2, 1]]
    skel, info = sc.thin_ref(sc.thin_cases()["pixel"], 64)
    assert skel.tolist() == [[[1]]] and info.tolist() == [[1, 1]]
    square = sc.thin_cases()["square40"]
    full, info = sc.thin_ref(square, 64)
    assert 18 <= info[0, 0] <= 22 and info[0, 1] == 1
    for cut in (1, 2):
        part, info = sc.thin_ref(square, cut)
        assert info.tolist() == [[cut, 0]] and part.sum() > full.sum()
    # a batch whose frames stop after different numbers of iterations
    _, info = sc.thin_ref(sc.thin_cases()["batch3"], 64)
    assert len(set(info[:, 0].tolist())) == 3 and info[2].tolist() == [1, 1]


def test_random_blobs_keep_their_components_and_never_vanish():
    for seed in range(12):
        m = sc.blob(5 + 5 * seed, 70 - 5 * seed, seed, 0.2 + 0.05 * seed)[None]
        skel, _ = sc.thin_ref(m)
        assert sc.count8(skel[0]) == sc.count8(m[0])


def test_annotator_restatement_strokes_every_large_error_region_inside_the_error():
    rng = np.random.RandomState(0)
    gt = np.stack([sc.blob(48, 64, 11, 0.3), sc.blob(48, 64, 12, 0.4)]).astype(np.uint8)
    pred = np.stack([sc.blob(48, 64, 13, 0.3), sc.blob(48, 64, 12, 0.4)]).astype(np.uint8)
    pred[1, 5:20, 5:25] ^= 1
    pred[1, 40, 60] ^= 1                     # a one-pixel error: below min_area
    out = sc.error_ref(pred, gt, min_area=16, keep_largest=False)
    err = pred != gt
    assert not ((out != 255) & ~err).any()
    assert ((out == gt) | (out == 255)).all()
    for n in range(2):
        lab = sc.components8(err[n])
        for i in np.unique(lab[lab > 0]):
            assert ((out[n] != 255) & (lab == i)).any() == ((lab == i).sum() >= 16)
    first = sc.initial_ref(gt)
    assert all((first[n] == 1).any() and (first[n] == 0).any() for n in range(2))
    assert ((first == gt) | (first == 255)).all()
    del rng


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------

def test_load_davis_json_rounds_half_up_and_clamps_into_the_frame():
    from osvos_pytorch_amd import scribble
    doc = {"scribbles": [[{"path": [[0.0, 0.0], [1.0, 1.0], [0.5, 0.5], [-0.2, 1.7]], "object_id": 1, "start_time": 0},
                          {"path": [[0.25, 0.75]], "object_id": 0}], [], [{"path": [], "object_id": 2}]]}
    paths, frames = scribble.load_davis_json(io.StringIO(json.dumps(doc)), (5, 11))
    assert frames == 3
    # W - 1 = 10: 0.5 -> 5; H - 1 = 4: 0.5 -> floor(2.5) = 2; 0.25 * 10 = 2.5 -> 3 (half up); 0.75 * 4 = 3
    assert paths == [(0, 1, [(0, 0), (10, 4), (5, 2), (0, 4)]), (0, 0, [(3, 3)])]
    table = scribble.segment_table(paths, frames)
    assert table.dtype == np.int32 and table.tolist() == [[0, 0, 10, 4, 1, 0], [10, 4, 5, 2, 1, 0], [5, 2, 0, 4, 1, 0], [3, 3, 3, 3, 0, 0]]
    for bad in ({}, {"scribbles": [[{"path": [[0.1]], "object_id": 1}]]}, {"scribbles": [[{"path": [[0.1, float("nan")]], "object_id": 1}]]},
                {"scribbles": [[{"path": [[0.1, 0.2]]}]]}):
        with pytest.raises(ValueError):
            scribble.davis_paths(bad, (5, 11))


def test_wrappers_refuse_bad_arguments_and_cpu_tensors():
    from osvos_pytorch_amd import scribble
    ok = [(0, 1, [(1, 2), (3, 4)])]
    for paths, frames in (([(1, 1, [(0, 0)])], 1), ([(0, 255, [(0, 0)])], 1), ([(0, -1, [(0, 0)])], 1), ([(0, 1, [])], 1), ([(0, 1, [(0, 16384)])], 1),
                          ([(0, 1, [(-1, 0)])], 1), ([(0, 1, [(0.5, 0)])], 1), ([(0, 1, [(0, 0, 0)])], 1), ([(0, 1)], 1), (ok, 0),
                          ([(0, 1, [(0, 0)] * 65537)], 1)):
        with pytest.raises(ValueError):
            scribble.segment_table(paths, frames)
    assert scribble.segment_table([], 1).shape == (0, 6)
    for kw in (dict(radius=-1), dict(radius=65), dict(radius=1.5), dict(size=(0, 4)), dict(size=(4, 16385)), dict(size=3)):
        with pytest.raises(ValueError):
            scribble.rasterize(ok, **dict(dict(size=(8, 8)), **kw))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scribble.rasterize(ok, (8, 8), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scribble.raster_segments(torch.zeros((1, 6), dtype=torch.int32), (8, 8))
    m = torch.zeros((1, 8, 8), dtype=torch.uint8)
    for call in (lambda: scribble.thin(m), lambda: scribble.initial_scribbles(m), lambda: scribble.error_scribbles(m, m),
                 lambda: scribble.training_planes(m[0], 1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for kw in (dict(max_iters=0), dict(max_iters=513), dict(path=3), dict(path=-1), dict(max_iters=True)):
        with pytest.raises(ValueError):
            scribble.check_thin(8, 8, **dict(dict(max_iters=64, path=0), **kw))
    scribble.check_thin(480, 854, 64, 1)                # 14 words x 480 rows fit
    scribble.check_thin(1080, 1920, 64, 0)
    with pytest.raises(ValueError, match="more than 8000"):
        scribble.check_thin(1080, 1920, 64, 1)
    with pytest.raises(ValueError):
        scribble.Robot(radius=65)
    with pytest.raises(ValueError):
        scribble.Robot(min_area=-1)


def test_the_library_refuses_bad_arguments_before_any_launch():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    p = C.c_void_p(4096)          # never dereferenced: every call below is refused before its launch

    def refused(rc, word):
        err = l.osvos_last_error()
        assert rc < 0 and word in err, (rc, err)

    def raster(segs=p, M=4, out=p, N=1, H=8, W=8, radius=3):
        return l.osvos_scribble_raster(segs, M, out, N, H, W, radius, None)

    def thin(mask=p, out=p, info=p, N=1, H=8, W=8, iters=4, path=0, ws=p):
        return l.osvos_mask_thin(mask, out, info, N, H, W, iters, path, ws, None)

    refused(raster(segs=None), b"null")
    refused(raster(out=None, M=0), b"null")
    refused(raster(M=-1), b"segments")
    refused(raster(M=65536), b"segments")
    refused(raster(N=0), b"N 0 frames")
    for kw in (dict(H=0), dict(W=16385)):
        refused(raster(**kw), b"bad size")
    for r in (-1, 65):
        refused(raster(radius=r), b"radius")
    for kw in (dict(mask=None), dict(out=None), dict(info=None), dict(ws=None)):
        refused(thin(**kw), b"null")
    for kw in (dict(N=0), dict(H=0), dict(W=16385), dict(N=65536)):
        refused(thin(**kw), b"frames")
    for it in (0, 513):
        refused(thin(iters=it), b"max_iters")
    for path in (-1, 3):
        refused(thin(path=path), b"path")
    refused(thin(H=1080, W=1920, path=1), b"path 1 keeps the plane in LDS")
    assert l.osvos_mask_thin_ws_bytes(0, 8, 8) == 0 and l.osvos_mask_thin_ws_bytes(1, 8, 16385) == 0
    assert l.osvos_mask_thin_ws_bytes(2, 480, 854) == 2 * 2 * 480 * 14 * 8 + 2 * 512 * 4
    assert (_lib.SCRIBBLE_LIST_CAP, _lib.THIN_RESIDENT_WORDS, _lib.THIN_MAX_ITERS) == (sc.LIST_CAP, 8000, 512)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "osvos_hip.h")).read()
    for name, v in (("OSVOS_SCRIBBLE_LIST_CAP", 512), ("OSVOS_THIN_RESIDENT_WORDS", 8000), ("OSVOS_THIN_MAX_ITERS", 512),
                    ("OSVOS_SCRIBBLE_MAX_SEGMENTS", 65535), ("OSVOS_SCRIBBLE_MAX_RADIUS", 64)):
        assert "#define %s %d\n" % (name, v) in hdr


def test_train_online_parses_and_refuses_before_gpu_work():
    import train_online as to
    base = ["--synthetic", "--device-augment", "--synthetic-frames", "3"]
    a = to.parse_args(base + ["--interactive", "2,3,2"])
    assert a.interactive == dict(rounds=2, steps0=3, steps=2, file="")
    assert to.parse_args(base + ["--interactive", "4"]).interactive == dict(rounds=4, steps0=200, steps=100, file="")
    assert to.parse_args(base + ["--scribbles", "s.json", "--scribble-radius", "5"]).interactive == dict(rounds=1, steps0=200, steps=100, file="s.json")
    assert to.parse_args(base + ["--interactive", "2", "--tta-flip", "--crf-iters", "2", "--snap-cell", "8"]).interactive["rounds"] == 2
    assert to.parse_args(base).interactive is None and to.parse_args(["--synthetic"]).interactive is None
    for extra in (["--multi-object"], ["--window-fused"], ["--lucid", "0.5"], ["--adapt-steps", "2"], ["--match-gain", "2"],
                  ["--match-gain", "2", "--match-previous"], ["--match-topk", "4"], ["--match-local", "2"], ["--match-memory", "64"],
                  ["--match-soft", "10"], ["--track-components", "8"], ["--zoom", "2"], ["--flow-search", "8"], ["--test-precision", "fp32h2"]):
        for opt in (["--interactive", "2"], ["--scribbles", "s.json"]):
            with pytest.raises(SystemExit) as e:
                to.parse_args(base + opt + extra)
            assert "is not run together with " + extra[0][:8] in str(e.value), (extra, str(e.value))
    for bad in (["--interactive", "0"], ["--interactive", "2,0"], ["--interactive", "2,3,4,5"], ["--interactive", "x"],
                ["--interactive", "2", "--scribble-radius", "65"], ["--interactive", "2", "--scribble-min-area", "-1"],
                ["--interactive", "2", "--scribble-prior", "-1"], ["--interactive", "2", "--scribbles", "s.json"]):
        with pytest.raises(SystemExit) as e:
            to.parse_args(base + bad)
        assert "--interactive" in str(e.value) or "--scribbles" in str(e.value)
    with pytest.raises(SystemExit, match="needs --device-augment"):
        to.parse_args(["--synthetic", "--interactive", "2"])
    assert to.parse_args(base + ["--interactive", "1", "--scribbles", "s.json"]).interactive["file"] == "s.json"


# ---- the session and the loop, with recording stand-ins ----------------------------------------------------------------------------------

class Loop(object):
    def __init__(self, rec):
        self.rec = rec

    def micro_batch(self, image, label, void_labels=False):
        assert void_labels and image.requires_grad
        self.rec.append(("micro_batch", int(image[0, 0, 0, 0]), label))
        return None, False


class Augment(object):
    def __init__(self, rec):
        self.rec, self.n = rec, 0

    def draw(self):
        self.n += 1
        self.rec.append(("draw", self.n))
        return bool(self.n % 2), 10.0 * self.n, 1.0


def make_session(monkeypatch, rec, frames=3, **kw):
    from osvos_pytorch_amd import scribble

    def planes(m, object_id, prev, prior):
        rec.append(("planes", prior, prev is not None))
        return (m != 255).to(torch.uint8) * 255, (m == object_id).to(torch.uint8) * 255

    def augment_frame(img, label, flip, rot, sc_, meanval=None):
        rec.append(("augment_frame", int(img[0, 0, 0]), None if label is None else int(label.max()), flip, rot, sc_))
        image = img.permute(2, 0, 1).float()
        return image, None if label is None else (label.float() / 255.0)[None]

    monkeypatch.setattr(scribble, "training_planes", planes)
    monkeypatch.setattr(scribble, "augment_frame", augment_frame)
    frames_u8 = [torch.full((4, 6, 3), f, dtype=torch.uint8) for f in range(frames)]
    return scribble.InteractiveSession(None, None, frames_u8, loop=Loop(rec), augment=Augment(rec), **kw)


def map_of(rows):
    return torch.tensor(rows, dtype=torch.uint8)


def test_session_merges_rotates_and_leaves_one_class_frames_out(monkeypatch):
    rec = []
    s = make_session(monkeypatch, rec, object_id=2, n_ave_grad=2)
    u = 255
    a = map_of([[2, 2, u, u, u, u], [u] * 6, [u, u, 0, 0, u, u], [u] * 6])
    assert s.add(1, a) is True
    assert s.add(0, map_of([[2] * 6] + [[u] * 6] * 3)) is False          # the object alone: one class
    assert s.add(2, map_of([[0] * 6] + [[u] * 6] * 3)) is False          # the background alone
    assert s.rotation == [1] and s.summary() == {"annotated": 3, "training": 1, "left_out": 2, "micro_batches": 0}
    # the merge: new labels overrule old ones, 255 never overrules
    assert s.add(1, map_of([[0, u, 2, u, u, u], [u] * 6, [u, u, u, 7, u, u], [u] * 6])) is True
    assert s.maps[1].tolist() == [[0, 2, 2, u, u, u], [u] * 6, [u, u, 0, 7, u, u], [u] * 6]
    assert s.add(2, map_of([[u] * 6] * 3 + [[u, u, u, u, u, 2]])) is True   # frame 2 now holds both
    assert s.rotation == [1, 2]                                            # in order of FIRST annotation: frame 0 is still out
    assert s.labelled_pixels() == 5 + 6 + 7
    with pytest.raises(ValueError):
        s.add(3, a)
    with pytest.raises(ValueError):
        s.add(0, a[:2])
    del rec[:]
    assert s.fit(2) == 4
    calls = [c[0] for c in rec]
    assert calls == ["planes", "draw", "augment_frame", "augment_frame", "micro_batch"] * 4
    assert [c[1] for c in rec if c[0] == "micro_batch"] == [1, 2, 1, 2]     # micro-batch k takes frame k mod A of the rotation
    warps = [c for c in rec if c[0] == "augment_frame"]
    for first, second in zip(warps[0::2], warps[1::2]):
        assert first[1] == second[1] and first[3:] == second[3:]          # the same frame under the same draw, twice
    assert [w[3:] for w in warps[0::2]] == [(True, 10.0, 1.0), (False, 20.0, 1.0), (True, 30.0, 1.0), (False, 40.0, 1.0)]
    label = [c for c in rec if c[0] == "micro_batch"][0][2]
    assert tuple(label.shape) == (1, 1, 4, 6)
    assert label[0, 0].tolist() == [[0, 1, 1, -1, -1, -1], [-1] * 6, [-1, -1, 0, 0, -1, -1], [-1] * 6]
    assert s.summary()["micro_batches"] == 4
    # nothing to train on: no step, no draw
    rec2 = []
    empty = make_session(monkeypatch, rec2)
    empty.add(0, map_of([[1] * 6] + [[u] * 6] * 3))
    assert empty.fit(3) == 0 and [c[0] for c in rec2] == []


class Session(object):
    """like scribble.InteractiveSession for the loop: records add and fit"""

    def __init__(self, rec, frames):
        self.rec, self.object_id = rec, 1
        self.frames_u8 = [torch.full((4, 6, 3), f, dtype=torch.uint8) for f in range(frames)]
        self.previous = None

    def add(self, frame, m):
        self.rec.append(("add", frame, int(m[0, 0])))

    def fit(self, steps):
        self.rec.append(("fit", steps))

    def image(self, frame):
        self.rec.append(("image", frame))
        return torch.full((1, 3, 4, 6), float(frame))

    def set_previous(self, masks):
        self.rec.append(("set_previous", len(masks)))

    def labelled_pixels(self):
        return 10 * len([c for c in self.rec if c[0] == "add"])


class Forward(object):
    needs_image = True

    def __init__(self, rec):
        self.rec = rec

    def __call__(self, frame_u8, image):
        self.rec.append(("forward", int(frame_u8[0, 0, 0]), int(image[0, 0, 0, 0])))
        return torch.full((1, 1, 4, 6), 1.0)

    def remember(self, out):
        self.rec.append(("remember",))


def test_loop_annotates_fits_predicts_and_scores_in_order():
    from osvos_pytorch_amd import sequence
    rec = []
    scores = iter([([0.9, 0.5, 0.2], [0.8, 0.4, 0.4]), ([0.9, 0.1, 0.6], [1.0, 0.5, 0.6]), ([1.0, 1.0, 1.0], [1.0, 1.0, 1.0])])

    class Evaluator(object):
        def __init__(self):
            rec.append(("evaluator",))

        def add(self, out, gt):
            rec.append(("score", float(gt.sum())))

        def per_frame(self):
            return next(scores)

    def robot(pred, gt):
        rec.append(("robot", None if pred is None else int(pred.max()), int(gt[0, 0])))
        return torch.full((4, 6), 9 if pred is None else 8, dtype=torch.uint8)

    def crf(fused, frame_u8):
        rec.append(("crf", int(frame_u8[0, 0, 0])))
        return fused

    gts = [torch.full((4, 6), f % 2, dtype=torch.uint8) for f in range(3)]
    lines = []
    report, fused = sequence.interactive_sequence(Session(rec, 3), Forward(rec), dict(crf=crf), 3, 7, 2, gts, robot, make_evaluator=Evaluator,
                                                  on_round=lambda r, rep: lines.append(r))
    predict = [("evaluator",)] + [c for f in range(3) for c in (("image", f), ("forward", f, f), ("crf", f), ("remember",), ("score", 24.0 * (f % 2)))] \
        + [("set_previous", 3)]
    assert rec == [("robot", None, 0), ("add", 0, 9), ("fit", 7)] + predict \
        + [("robot", 1, 0), ("add", 2, 8), ("fit", 2)] + predict \
        + [("robot", 1, 1), ("add", 1, 8), ("fit", 2)] + predict          # the frame of the lowest J of the round before: 2, then 1
    assert [r["frame"] for r in report] == [0, 2, 1] and lines == [0, 1, 2]
    assert [r["labelled"] for r in report] == [10, 20, 30]
    assert report[0]["J"] == pytest.approx((0.9 + 0.5 + 0.2) / 3) and report[1]["F"] == pytest.approx(0.7)
    assert len(fused) == 3 and all(r["fit_s"] >= 0 and r["predict_s"] >= 0 for r in report)
    # a person's strokes open the first round in place of the robot's
    del rec[:]
    scores = iter([([1.0] * 3, [1.0] * 3)])
    first = [(1, torch.full((4, 6), 5, dtype=torch.uint8)), (2, torch.full((4, 6), 6, dtype=torch.uint8))]
    report, _ = sequence.interactive_sequence(Session(rec, 3), Forward(rec), {}, 1, 4, 2, gts, robot, first=first, make_evaluator=Evaluator)
    assert rec[:3] == [("add", 1, 5), ("add", 2, 6), ("fit", 4)] and not any(c[0] == "robot" for c in rec) and report[0]["frame"] == [1, 2]
    with pytest.raises(ValueError):
        sequence.interactive_sequence(Session(rec, 3), Forward(rec), {}, 0, 4, 2, gts, robot)
    with pytest.raises(ValueError):
        sequence.interactive_sequence(Session(rec, 3), Forward(rec), {}, 1, 4, 2, gts[:2] + [None], robot)
