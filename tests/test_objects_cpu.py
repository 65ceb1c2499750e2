"""CPU: the host side of the multi-object (DAVIS 2017) results path -- the three ABI symbols of csrc/objects.hip, the indexed PNG writer and
the DAVIS palette, DavisFrames(indexed=True), the arithmetic of MultiObjectEvaluator.summary on a hand-filled count table, the argument
check of train_online.py --multi-object, and the fixture tests/golden/objects.npz against a restatement of the merge."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import object_cases as oc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("osvos_merge_objects", "osvos_labels_jf_ws_bytes", "osvos_labels_jf_counts")


def test_the_three_symbols_are_declared_prototyped_and_exported():
    from osvos_pytorch_amd import _lib
    hdr = open(os.path.join(REPO, "include", "osvos_hip.h")).read()
    declared = set(re.findall(r"\b(osvos_[a-z0-9_]+)\s*\(", hdr))
    l = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (osvos_[a-z0-9_]+)$", nm, re.M))
    for s in SYMBOLS:
        assert s in declared and s in _lib.PROTOTYPES and s in exported and hasattr(l, s), s
    m = re.search(r"#define\s+OSVOS_MAX_OBJECTS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == 16 == _lib.MAX_OBJECTS
    # the size query is host arithmetic: two one-bit maps per frame and object, rows padded to 64-pixel words
    assert l.osvos_labels_jf_ws_bytes(3, 10, 480, 854) == 2 * 3 * 10 * 480 * 14 * 8
    assert l.osvos_labels_jf_ws_bytes(1, 1, 1, 1) == 16
    assert l.osvos_labels_jf_ws_bytes(1, 17, 8, 8) == 0 and l.osvos_labels_jf_ws_bytes(0, 1, 8, 8) == 0


def test_argument_errors_need_no_device():
    from osvos_pytorch_amd import _lib
    l = _lib.lib()
    assert l.osvos_merge_objects(None, None, 1, 1, 8, 8, 0.0, None) < 0 and b"null" in l.osvos_last_error()
    assert l.osvos_labels_jf_counts(None, None, None, None, 1, 1, 8, 8, 1, 0, None) < 0 and b"null" in l.osvos_last_error()


def test_davis_palette_is_the_pascal_voc_colour_map():
    from osvos_pytorch_amd import results
    pal = results.davis_palette()
    assert pal.shape == (256, 3) and pal.dtype == np.uint8
    assert pal[:5].tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128]]
    assert pal[7].tolist() == [128, 128, 128] and pal[8].tolist() == [64, 0, 0] and pal[15].tolist() == [192, 128, 128]
    assert pal[255].tolist() == [224, 224, 192]
    assert len(set(map(tuple, pal.tolist()))) == 256


def test_indexed_png_reads_back_with_pillow(tmp_path):
    from PIL import Image
    from osvos_pytorch_amd import results
    rng = np.random.default_rng(0)
    for (h, w, top) in [(37, 53, 4), (1, 1, 1), (48, 64, 256)]:
        lab = rng.integers(0, top, size=(h, w)).astype(np.uint8)
        path = str(tmp_path / ("l_%d_%d.png" % (h, w)))
        results.write_indexed_png(path, lab)
        with Image.open(path) as im:
            assert im.mode == "P" and im.size == (w, h)
            assert np.array_equal(np.asarray(im), lab)
            assert np.array_equal(np.asarray(im.getpalette(), dtype=np.uint8).reshape(-1, 3), results.davis_palette())
    # a palette of one's own; a label beyond it is an error, not a wrong colour
    own = np.array([[1, 2, 3], [4, 5, 6]], dtype=np.uint8)
    path = str(tmp_path / "own.png")
    results.write_indexed_png(path, np.array([[0, 1], [1, 0]], dtype=np.uint8), own)
    with Image.open(path) as im:
        assert np.asarray(im.convert("RGB")).tolist() == [[[1, 2, 3], [4, 5, 6]], [[4, 5, 6], [1, 2, 3]]]
    with pytest.raises(ValueError):
        results.write_indexed_png(path, np.array([[0, 2]], dtype=np.uint8), own)
    with pytest.raises(ValueError):
        results.write_indexed_png(path, np.zeros((2, 2, 2), dtype=np.uint8))
    # save_label_maps: one file per frame (host arrays take the same route as a device tensor after its one copy)
    maps = rng.integers(0, 3, size=(2, 5, 7)).astype(np.uint8)
    paths = [str(tmp_path / ("f%d.png" % i)) for i in range(2)]
    results.save_label_maps(maps, paths)
    for p, m in zip(paths, maps):
        with Image.open(p) as im:
            assert im.mode == "P" and np.array_equal(np.asarray(im), m)
    # the grayscale writer is untouched by the shared encoder
    g = rng.integers(0, 256, size=(9, 11)).astype(np.uint8)
    results.write_png(str(tmp_path / "g.png"), g)
    with Image.open(str(tmp_path / "g.png")) as im:
        assert im.mode == "L" and np.array_equal(np.asarray(im), g)


def _davis_tree(root, seq, n_frames, n_annot, h=12, w=20):
    from PIL import Image
    from osvos_pytorch_amd import results
    os.makedirs(os.path.join(root, "JPEGImages", "480p", seq))
    os.makedirs(os.path.join(root, "Annotations", "480p", seq))
    rng = np.random.default_rng(3)
    labs = []
    for i in range(n_frames):
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8)).save(os.path.join(root, "JPEGImages", "480p", seq, "%05d.jpg" % i))
    for i in range(n_annot):
        lab = rng.integers(0, 4, size=(h, w)).astype(np.uint8)
        im = Image.frombytes("P", (w, h), lab.tobytes())
        im.putpalette(results.davis_palette().reshape(-1).tolist())
        im.save(os.path.join(root, "Annotations", "480p", seq, "%05d.png" % i))
        labs.append(lab)
    return labs


def test_davis_frames_indexed_returns_raw_indices_and_every_annotation(tmp_path):
    from PIL import Image
    from osvos_pytorch_amd.davis_io import DavisFrames, n_objects
    root = str(tmp_path)
    labs = _davis_tree(root, "dogs", 4, 3)          # the last frame has no annotation on disk
    test = DavisFrames(False, root, seq_name="dogs", indexed=True)
    assert len(test) == 4
    for i in range(3):
        img, lab = test[i]
        assert img.shape == (12, 20, 3) and lab.dtype == np.uint8 and np.array_equal(lab, labs[i])
    assert test[3][1] is None
    assert n_objects(test[0][1]) == int(labs[0].max()) == 3
    train = DavisFrames(True, root, seq_name="dogs", indexed=True)
    assert len(train) == 1 and np.array_equal(train[0][1], labs[0])
    # the default is what it was: first annotation only, read through convert('L') (the palette's grey values, not the indices)
    old = DavisFrames(False, root, seq_name="dogs")
    assert old.labels[1:] == [None, None, None] and old.indexed is False
    with Image.open(os.path.join(root, "Annotations", "480p", "dogs", "00000.png")) as im:
        want = np.asarray(im.convert("L"))
    assert np.array_equal(old[0][1], want) and not np.array_equal(want, labs[0])
    assert old[1][1] is None and np.array_equal(old[1][0], test[1][0])
    # a non-palette annotation is returned as before, also when indexed
    Image.fromarray((labs[0] > 0).astype(np.uint8) * 255).save(os.path.join(root, "Annotations", "480p", "dogs", "00000.png"))
    assert np.array_equal(DavisFrames(False, root, seq_name="dogs", indexed=True)[0][1], (labs[0] > 0).astype(np.uint8) * 255)


def test_multi_object_evaluator_summary_arithmetic_from_a_host_table():
    from osvos_pytorch_amd import results
    ev = results.MultiObjectEvaluator(2)
    # frames x objects x {inter, union, n_fb, n_gb, fb_match, gb_match}
    table = np.array([[[50, 100, 10, 10, 10, 10], [0, 0, 0, 0, 0, 0]],
                      [[30, 120, 20, 10, 10, 5], [10, 40, 0, 8, 0, 0]],
                      [[90, 100, 10, 20, 5, 20], [20, 40, 6, 0, 0, 0]],
                      [[0, 50, 12, 12, 0, 0], [40, 40, 8, 8, 8, 8]]], dtype=np.int64)
    ev.frames, ev._host = 4, (4, table)
    per = ev.per_object()
    assert per[0][0] == [0.5, 0.25, 0.9, 0.0] and per[1][0] == [1.0, 0.25, 0.5, 1.0]
    assert per[0][1] == [1.0, 0.5, 2 * 0.5 * 1.0 / 1.5, 0.0] and per[1][1] == [1.0, 0.0, 0.0, 1.0]
    s = ev.summary()
    assert s["frames"] == 4 and len(s["objects"]) == 2
    for o, (js, fs) in zip(s["objects"], per):
        assert o["J"] == results.davis_statistics(js) and o["F"] == results.davis_statistics(fs)
        assert o["J&F"] == 0.5 * (o["J"]["mean"] + o["F"]["mean"])
    assert s["J"] == pytest.approx((np.mean(per[0][0]) + np.mean(per[1][0])) / 2, abs=1e-15)
    assert s["F"] == pytest.approx((np.mean(per[0][1]) + np.mean(per[1][1])) / 2, abs=1e-15)
    assert s["J&F"] == 0.5 * (s["J"] + s["F"])
    e = ev.summary(exclude_ends=True)
    assert e["frames"] == 2
    assert e["objects"][0]["J"] == results.davis_statistics([0.25, 0.9]) and e["objects"][1]["F"] == results.davis_statistics([0.0, 0.0])
    assert e["J"] == pytest.approx((0.575 + 0.375) / 2, abs=1e-15) and e["F"] == pytest.approx((0.5 + 2.0 / 3.0) / 2 / 2, abs=1e-15)
    ev.frames, ev._host = 2, (2, table[:2])
    with pytest.raises(ValueError, match="at least 3 frames"):
        ev.summary(exclude_ends=True)
    with pytest.raises(ValueError, match="at least 1 frames"):
        results.MultiObjectEvaluator(2).summary()
    with pytest.raises(ValueError):
        results.MultiObjectEvaluator(17)
    with pytest.raises(ValueError):
        results.MultiObjectEvaluator(0)


def test_train_online_multi_object_needs_the_device_pipeline():
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "train_online.py", "--multi-object"], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "--multi-object needs --device-augment or --synthetic" in r.stderr, r.stderr[-2000:]


def _merge(x, t):
    """the definition of include/osvos_hip.h, pixel by pixel in plain Python"""
    k, n, h, w = x.shape
    out = np.zeros((n, h, w), dtype=np.uint8)
    flat, o = x.reshape(k, -1), out.reshape(-1)
    for i in range(flat.shape[1]):
        best, who = None, 0
        for j in range(k):
            v = flat[j, i]
            if v == v and (best is None or v > best):
                best, who = v, j + 1
        o[i] = who if best is not None and best > t else 0
    return out


def test_fixture_covers_what_it_must_and_its_label_maps_are_the_merge_of_its_logits():
    cases = oc.load()
    assert sorted(set(c["K"] for c in cases)) == [1, 2, 3, 10, 16]
    assert {85, 107} <= set(c["W"] for c in cases) and any((c["H"], c["W"]) == (480, 854) for c in cases)
    assert sum(1 for c in cases if (c["special"][:, 3] == oc.TIE).any()) >= 3
    kinds = set(int(v) for c in cases for v in c["special"][:, 3])
    assert kinds == {oc.TIE, oc.THR_EQ, oc.NAN, oc.ALL_NAN}
    assert any(c["thr"] != 0.5 for c in cases)
    assert any(int(c["gt"].max()) > c["K"] for c in cases)                                  # ids above K
    absent_p = absent_g = absent_both = False
    for c in cases:
        assert c["counts"].shape == (c["N"], c["K"], 6) and int(c["pred"].max()) <= c["K"]
        for n in range(c["N"]):
            for k in range(1, c["K"] + 1):
                p, g = bool((c["pred"][n] == k).any()), bool((c["gt"][n] == k).any())
                absent_p |= g and not p
                absent_g |= p and not g
                absent_both |= not p and not g
                # the region counts are plain pixel counts: checked here without the generator
                assert c["counts"][n, k - 1, 0] == int(((c["pred"][n] == k) & (c["gt"][n] == k)).sum())
                assert c["counts"][n, k - 1, 1] == int(((c["pred"][n] == k) | (c["gt"][n] == k)).sum())
    assert absent_p and absent_g and absent_both
    for c in cases:
        if c["H"] * c["W"] > 10000:
            continue                                  # (the pixel loop is Python; the generator asserts the same for every case)
        x = oc.logits(c)
        assert x.dtype == np.float32 and x.shape == (c["K"], c["N"], c["H"], c["W"])
        assert np.array_equal(_merge(x, oc.logit_threshold(c["thr"])), c["pred"]), c["name"]
        for n, y, xx, kind, a, b in c["special"]:
            if kind == oc.TIE:
                assert x[a - 1, n, y, xx] == x[b - 1, n, y, xx] == np.nanmax(x[:, n, y, xx]) and c["pred"][n, y, xx] == a < b
            elif kind == oc.THR_EQ:
                assert np.nanmax(x[:, n, y, xx]) == oc.logit_threshold(c["thr"]) and c["pred"][n, y, xx] == 0
            elif kind == oc.NAN:
                assert np.isnan(x[a - 1, n, y, xx]) and c["pred"][n, y, xx] != a
            else:
                assert np.isnan(x[:, n, y, xx]).all() and c["pred"][n, y, xx] == 0
