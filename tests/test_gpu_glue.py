"""GPU: the stage wrappers launch on the device of their tensors, whatever the current device is (osvos_pytorch_amd._glue.call).  Each of the
eight wrappers that used to take the current device's stream runs on seeded inputs that live on cuda:1 while cuda:0 stays current; the result
must live on cuda:1 and equal, bit for bit, the same call made with the inputs on cuda:0.  N = 2, H = 13, W = 18: the odd width takes the
kernels' scalar-store path.  Needs two GPUs."""
import numpy as np
import pytest
import torch

from osvos_pytorch_amd import adapt, augment, results, roi, tta

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")]

N, H, W = 2, 13, 18
CANVAS = (11, 15)


def _inputs():
    """seeded host tensors: decoded frames, an object mask per frame, a logit map per frame at the frame's and at the canvas's size"""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[:H, :W]
    mask = np.stack([((xx - 6 - 4 * n) ** 2 + (yy - 5) ** 2 <= 9) for n in range(N)])
    return dict(frames=torch.from_numpy(rng.integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)), mask=torch.from_numpy(mask),
                logits=torch.from_numpy(rng.normal(0, 4, size=(N, 1, H, W)).astype(np.float32)),
                small=torch.from_numpy(rng.normal(0, 4, size=(N, 1) + CANVAS).astype(np.float32)))


def _stages(t):
    """name -> result tensors of the eight wrappers on the tensors of ``t`` (all on one device)"""
    box = roi.mask_box(t["mask"], CANVAS, margin_pct=0, margin_px=1, max_zoom=4.0)          # (0, 1, 13, 9) and (4, 1, 13, 9): real crops
    return {"tta.make_view": [tta.make_view(t["frames"], 10, 23, flip=True)],
            "tta.fuse_views": [tta.fuse_views([t["logits"], t["small"]], [False, True], (H, W), weights=[0.75, 0.25])],
            "roi.mask_box": [box],
            "roi.crop_view": [roi.crop_view(t["frames"], box, CANVAS)],
            "roi.paste": [roi.paste(t["small"], box, (H, W))],
            "results.mask_bytes": [results.mask_bytes(t["logits"])],
            "adapt.adaptation_targets": list(adapt.adaptation_targets(t["logits"], t["mask"], prob=0.6, erosion=1, distance=4)),
            "augment.augment_frame": list(augment.augment_frame(t["frames"][0], t["mask"][0].to(torch.uint8) * 255, True, 17.0, 1.1))}


def test_wrappers_launch_on_the_device_of_their_tensors():
    host = _inputs()
    torch.cuda.set_device(0)
    want = _stages({k: v.to("cuda:0") for k, v in host.items()})
    got = _stages({k: v.to("cuda:1") for k, v in host.items()})
    assert torch.cuda.current_device() == 0
    torch.cuda.synchronize(0)
    torch.cuda.synchronize(1)
    for name in want:
        assert len(got[name]) == len(want[name]), name
        for a, b in zip(got[name], want[name]):
            assert a.device == torch.device("cuda:1") and b.device == torch.device("cuda:0"), name
            assert a.dtype == b.dtype and a.shape == b.shape, name
            assert np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8)), name
    assert want["roi.mask_box"][0].cpu().tolist() == [[0, 1, 13, 9], [4, 1, 13, 9]]
