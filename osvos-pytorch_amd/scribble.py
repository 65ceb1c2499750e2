"""Interactive scribbles (Scribble-OSVOS, the baseline of the DAVIS interactive track): the network is fine-tuned on the pixels a user's strokes
label, everything else is void; a simulated annotator looks at the worst frame and draws strokes through its largest errors; repeat.

``rasterize`` turns strokes (host polylines) into a label map on the device (``osvos_scribble_raster``: 255 = unlabelled, else the value of the
covering segment of the highest index, so later strokes overrule earlier ones); ``thin`` is the Guo-Hall skeleton of a mask
(``osvos_mask_thin``), the stroke of a region; include/osvos_hip.h states both rules.  ``initial_scribbles`` and ``error_scribbles`` are the
simulated annotator, made of those two, ``results.filter_components`` and ``results.distance_map`` with plain torch comparisons in between;
``training_planes`` turns a label map into the two two-valued planes ``augment.augment_frame`` warps with its nearest-neighbour rule;
``InteractiveSession`` keeps the merged strokes of every annotated frame and trains on them through ``TrainLoop.micro_batch(void_labels=True)``.
``sequence.interactive_sequence`` is the loop around it.  Everything is enqueued; the read-backs are one per ``InteractiveSession.add`` and
one per ``initial_scribbles`` (which values the annotation holds), at interaction rate, not frame rate.

``load_davis_json`` reads the scribble layout of the DAVIS interactive challenge.  The ``davisinteractive`` package was not available where
this was written: the layout is taken from its published description, and NO parity with that package's own rasteriser or robot is claimed.
"""
import json

import numpy as np
import torch

from . import _glue as g
from ._lib import SCRIBBLE_MAX_RADIUS, SCRIBBLE_MAX_SEGMENTS, SQDIST_MAX_SIDE, THIN_MAX_ITERS, THIN_RESIDENT_WORDS, lib
from .augment import MEANVAL, augment_frame
from .results import distance_map, filter_components
from .train_common import TrainLoop

UNLABELLED = 255          # the byte of a pixel no stroke covers
MAX_SIDE = 16384          # coordinates and sides stay below 2^14: the coverage rule is exact in int64 (include/osvos_hip.h)


def _size(size, what, max_side=MAX_SIDE):
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError("%s takes a size (H, W), got %r" % (what, size))
    if not (1 <= h <= max_side and 1 <= w <= max_side):
        raise ValueError("%s %d x %d: every side is 1..%d" % (what, h, w, max_side))
    return h, w


def segment_table(paths, frames=1):
    """paths: a host list of (frame, value, points) -- frame 0..frames - 1, value 0..254 (0 = background, others object ids), points a
    sequence of integer pixel (x, y) in [0, 16384) -> int32 numpy [M,6], one row (x0, y0, x1, y1, value, frame) per segment, in the order
    given; a path of one point gives one degenerate segment.  ValueError on anything else, and on more than 65535 segments."""
    g.check_int("frames", frames, 1, 65535, "scribble")
    rows = []
    for i, path in enumerate(paths):
        try:
            frame, value, points = path
            points = [tuple(p) for p in points]
        except (TypeError, ValueError):
            raise ValueError("scribble: path %d must be (frame, value, points), got %r" % (i, path))
        g.check_int("frame of path %d" % i, frame, 0, frames - 1, "scribble")
        g.check_int("value of path %d" % i, value, 0, UNLABELLED - 1, "scribble")
        if not points:
            raise ValueError("scribble: path %d has no point" % i)
        for p in points:
            if len(p) != 2:
                raise ValueError("scribble: path %d: a point is (x, y), got %r" % (i, p))
            for c in p:
                g.check_int("a coordinate of path %d" % i, c, 0, MAX_SIDE - 1, "scribble")
        pairs = [(points[0], points[0])] if len(points) == 1 else zip(points[:-1], points[1:])
        rows += [(int(a[0]), int(a[1]), int(b[0]), int(b[1]), int(value), int(frame)) for a, b in pairs]
    if len(rows) > SCRIBBLE_MAX_SEGMENTS:
        raise ValueError("scribble: %d segments; one call takes at most %d" % (len(rows), SCRIBBLE_MAX_SEGMENTS))
    return np.asarray(rows, dtype=np.int32).reshape(len(rows), 6)


def check_radius(radius):
    g.check_int("radius", radius, 0, SCRIBBLE_MAX_RADIUS, "scribble")


def raster_segments(segs, size, radius=3, frames=1, out=None):
    """segs: int32 CUDA tensor [M,6] (``segment_table``'s rows; a row with frame < 0 is padding) -> uint8 [frames,H,W].  The kernel does not
    check coordinates or values: ``segment_table`` does.  out: a contiguous uint8 [frames,H,W] tensor to write into."""
    g.need_cuda(segs, "segs", "scribble")
    if segs.dtype != torch.int32 or segs.dim() != 2 or segs.shape[1] != 6 or segs.shape[0] > SCRIBBLE_MAX_SEGMENTS:
        raise ValueError("segs must be an int32 [M,6] tensor of at most %d rows, got %s %s" % (SCRIBBLE_MAX_SEGMENTS, segs.dtype, tuple(segs.shape)))
    h, w = _size(size, "the frame size")
    check_radius(radius)
    g.check_int("frames", frames, 1, 65535, "scribble")
    segs = segs.contiguous()
    out = g.out_buffer(out, torch.uint8, (frames, h, w), segs.device, "the segments' device", module="scribble")
    m = int(segs.shape[0])
    g.call("scribble_raster", segs.device, g.ptr(segs) if m else None, m, g.ptr(out), frames, h, w, int(radius))
    return out


def rasterize(paths, size, radius=3, frames=1, device="cuda", out=None):
    """paths: ``segment_table``'s host list of (frame, value, points); size: (H, W) -> uint8 CUDA tensor [frames,H,W]: 255 where no stroke of
    the frame comes within ``radius`` pixels (0..64; a disc around every segment), else the value of the LAST such stroke segment.  The
    segment table is built and checked on the host and uploaded (an upload, not a read-back), then rastered in one launch."""
    table = segment_table(paths, frames)
    _size(size, "the frame size")
    check_radius(radius)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("osvos_pytorch_amd.scribble needs a CUDA (ROCm) device (%s); there is no CPU fallback" % device)
    return raster_segments(torch.from_numpy(table).to(device), size, radius, frames, out)


def davis_paths(doc, size):
    """the DAVIS interactive scribble document ``{"scribbles": [per frame: [{"path": [[x, y], ..], "object_id": k, ..}, ..]]}``, x and y
    normalised to [0, 1] -> (``segment_table``'s path list, the frame count).  A pixel coordinate is floor(x (W - 1) + 0.5), clamped into
    the frame.  No parity with the ``davisinteractive`` package is claimed (module docstring)."""
    h, w = _size(size, "the frame size")
    try:
        per_frame = list(doc["scribbles"])
    except (TypeError, KeyError):
        raise ValueError('scribble: the document has no "scribbles" list')
    paths = []
    for f, strokes in enumerate(per_frame):
        for s in strokes:
            try:
                value, pts = int(s["object_id"]), [(float(x), float(y)) for x, y in s["path"]]
            except (TypeError, KeyError, ValueError):
                raise ValueError('scribble: a stroke of frame %d is not {"path": [[x, y], ..], "object_id": k}' % f)
            if not all(np.isfinite(x) and np.isfinite(y) for x, y in pts):
                raise ValueError("scribble: a stroke of frame %d has a coordinate that is not finite" % f)
            if pts:
                paths.append((f, value, [(min(max(int(np.floor(x * (w - 1) + 0.5)), 0), w - 1), min(max(int(np.floor(y * (h - 1) + 0.5)), 0), h - 1))
                                         for x, y in pts]))
    return paths, len(per_frame)


def load_davis_json(file, size):
    """``davis_paths`` of a JSON file (a path or an open file) -> (paths, frames)"""
    if hasattr(file, "read"):
        return davis_paths(json.load(file), size)
    with open(file) as fh:
        return davis_paths(json.load(fh), size)


def check_thin(h, w, max_iters, path):
    """ValueError unless max_iters is 1..512, path 0 (automatic), 1 (resident) or 2 (global), and path 1's plane fits: H ceil(W / 64) <= 8000"""
    g.check_int("max_iters", max_iters, 1, THIN_MAX_ITERS, "thin")
    g.check_int("path", path, 0, 2, "thin")
    words = int(h) * (-(-int(w) // 64))
    if path == 1 and words > THIN_RESIDENT_WORDS:
        raise ValueError("thin: path 1 keeps the 1-bit plane in LDS: %d x %d is %d words, more than %d" % (h, w, words, THIN_RESIDENT_WORDS))


def thin(mask, max_iters=64, path=0, out=None):
    """mask: uint8 or bool CUDA tensor [N,H,W], [N,1,H,W] or [H,W] (non-zero = set) -> (skeleton uint8 [N,H,W] in {0, 1}, info int32 [N,2] on the
    device: iterations run, 1 if the last of them deleted nothing).  The Guo-Hall rule of include/osvos_hip.h: the skeleton is a subset of
    the mask, keeps its 8-connected components and never empties one.  path: 0 automatic, 1 the LDS-resident kernel, 2 the global one;
    both give the same bytes.  Enqueued only.  out: a contiguous uint8 [N,H,W] tensor to write into (it may be the mask)."""
    g.need_cuda(mask, "mask", "scribble")
    mask, n, h, w = g.planes(mask, "mask", (torch.uint8, torch.bool), max_side=MAX_SIDE)
    check_thin(h, w, max_iters, path)
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    out = g.out_buffer(out, torch.uint8, (n, h, w), mask.device, "the mask's device", module="scribble")
    info = torch.empty((n, 2), device=mask.device, dtype=torch.int32)
    ws = g.workspace(lib().osvos_mask_thin_ws_bytes(n, h, w), mask.device, what="%d frames of %d x %d" % (n, h, w), prefix="thin", dtype=torch.int64)
    g.call("mask_thin", mask.device, g.ptr(mask), g.ptr(out), g.ptr(info), n, h, w, int(max_iters), int(path), g.ptr(ws))
    return out, info


def _labels(t, what):
    g.need_cuda(t, what, "scribble")
    t, n, h, w = g.planes(t, what, (torch.uint8,), max_side=SQDIST_MAX_SIDE, dims=(2, 3))
    return t.view(n, h, w), n, h, w


def _stroke(region, radius, max_iters):
    """region: bool [N,H,W] -> bool: the pixels of the kept part of ``region`` within ``radius`` of its skeleton"""
    skeleton, _ = thin(region, max_iters)
    return region & (distance_map(skeleton) <= radius * radius)


def _largest(region):
    """bool [N,H,W] -> bool: the largest 8-connected component of every frame (the lowest label on a tie)"""
    pm = torch.where(region, 1.0, -1.0)
    return filter_components(pm, connectivity=8, keep_largest=True)[1] != 0


def initial_scribbles(gt_labels, radius=3, max_iters=THIN_MAX_ITERS):
    """The first interaction: gt_labels uint8 CUDA [N,H,W] or [H,W] -> uint8 [N,H,W].  (max_iters defaults to the largest, 512: a whole
    object or the background around it is hundreds of pixels thick, and a run cut short leaves a blob, not a stroke.)  For every value the annotation holds (background 0
    included; which ones: one 256-count read-back) the skeleton of the largest 8-connected component of that value, widened to ``radius``
    inside the component, carries the value; everything else is 255.  An annotation with an object therefore always yields both classes."""
    gt, n, h, w = _labels(gt_labels, "gt_labels")
    check_radius(radius)
    g.check_int("max_iters", max_iters, 1, THIN_MAX_ITERS, "thin")
    out = torch.full_like(gt, UNLABELLED)
    present = torch.bincount(gt.reshape(-1).long(), minlength=256).cpu().numpy()
    for v in np.nonzero(present[:UNLABELLED])[0]:
        region = _largest(gt == int(v))
        out = torch.where(_stroke(region, int(radius), max_iters), torch.full_like(gt, int(v)), out)
    return out


def error_scribbles(pred_labels, gt_labels, min_area=64, keep_largest=True, radius=3, max_iters=64):
    """The simulated annotator: pred_labels, gt_labels uint8 CUDA [N,H,W] or [H,W] -> uint8 [N,H,W].  E = pred != gt; the kept components of
    E are ``results.filter_components``' on a +-1 map with ``min_area`` / ``keep_largest``; S = thin(kept); the output is gt where kept and
    within ``radius`` of S, 255 elsewhere: a stroke carries the TRUE label of the error it runs through.  Enqueued only."""
    pred, n, h, w = _labels(pred_labels, "pred_labels")
    gt, n2, h2, w2 = _labels(gt_labels, "gt_labels")
    if (n, h, w) != (n2, h2, w2) or pred.device != gt.device:
        raise ValueError("scribble: prediction %s and annotation %s differ" % (tuple(pred_labels.shape), tuple(gt_labels.shape)))
    check_radius(radius)
    g.check_int("min_area", min_area, 0, 2 ** 31 - 1, "scribble")
    g.check_int("max_iters", max_iters, 1, THIN_MAX_ITERS, "thin")
    pm = torch.where(pred != gt, 1.0, -1.0)
    kept = filter_components(pm, connectivity=8, min_area=int(min_area), keep_largest=bool(keep_largest))[1] != 0
    return torch.where(_stroke(kept, int(radius), max_iters), gt, torch.full_like(gt, UNLABELLED))


def training_planes(scribble_map, object_id, prev_mask=None, prior_distance=0):
    """scribble_map: uint8 CUDA [H,W] -> (labelled, labelled_object): two uint8 [H,W] planes in {0, 255}.  A pixel is labelled when a stroke
    covers it, and labelled object when that stroke's value is ``object_id``.  With ``prior_distance`` D > 0 and ``prev_mask`` (the previous
    round's mask, non-zero = object) an unlabelled pixel farther than D from every stroke takes the previous prediction as its label; nearer
    ones stay void.  Each plane is two-valued, so ``augment_frame`` warps it with its nearest-neighbour rule."""
    g.need_cuda(scribble_map, "scribble_map", "scribble")
    m, _, h, w = g.planes(scribble_map, "scribble_map", (torch.uint8,), max_side=SQDIST_MAX_SIDE, dims=(2,))
    g.check_int("object_id", object_id, 1, UNLABELLED - 1, "scribble")
    g.check_int("prior_distance", prior_distance, 0, 2 * SQDIST_MAX_SIDE, "scribble")
    labelled, obj = m != UNLABELLED, m == int(object_id)
    if prior_distance > 0 and prev_mask is not None:
        g.need_cuda(prev_mask, "prev_mask", "scribble")
        if prev_mask.numel() != h * w or tuple(prev_mask.shape[-2:]) != (h, w):
            raise ValueError("prev_mask %s does not fit the %d x %d map" % (tuple(prev_mask.shape), h, w))
        far = ~labelled & (distance_map(labelled)[0] > int(prior_distance) ** 2)
        labelled, obj = labelled | far, obj | (far & (prev_mask.reshape(h, w) != 0))
    return labelled.to(torch.uint8) * 255, obj.to(torch.uint8) * 255


def merge_labels(old, new):
    """the merge rule of ``InteractiveSession.add``: new labels overrule old ones, 255 never overrules (plain torch, any device)"""
    return new.clone() if old is None else torch.where(new != UNLABELLED, new, old)


class Robot(object):
    """The simulated annotator as the loop calls it: ``robot(None, gt)`` -> the first interaction (``initial_scribbles``),
    ``robot(pred, gt)`` -> ``error_scribbles`` (``max_iters`` is the error strokes'; the first interaction thins to the end); maps [H,W]
    in, map [H,W] out.  The defaults are starting values, not tuned on DAVIS."""

    def __init__(self, radius=3, min_area=64, keep_largest=True, max_iters=64):
        check_radius(radius)
        g.check_int("min_area", min_area, 0, 2 ** 31 - 1, "scribble")
        g.check_int("max_iters", max_iters, 1, THIN_MAX_ITERS, "thin")
        self.radius, self.min_area, self.keep_largest, self.max_iters = radius, min_area, keep_largest, max_iters

    def __call__(self, pred_labels, gt_labels):
        if pred_labels is None:
            return initial_scribbles(gt_labels, self.radius)[0]
        return error_scribbles(pred_labels, gt_labels, self.min_area, self.keep_largest, self.radius, self.max_iters)[0]


class InteractiveSession(object):
    """The strokes of a sequence and the training on them.  frames_u8: the decoded frames, a uint8 CUDA tensor [F,H,W,3] or a list of [H,W,3].

    ``add(frame, scribble_map)`` merges a uint8 [H,W] map into that frame's (``merge_labels``) and decides, with ONE small read-back, whether
    the frame's merged labels hold both classes -- ``object_id`` and anything else labelled.  Only such a frame is in the training rotation:
    under the class-balanced loss the weight of a class is the other class's share of the labelled pixels (csrc/loss.hip, cbce_weights), so
    a sample with one class has weight 0 on every labelled pixel and contributes exactly nothing -- loss 0, gradient 0 -- and a step on it
    would only spend time.  ``summary()`` counts the frames left out.

    ``fit(steps)`` runs ``steps`` optimizer steps of ``n_ave_grad`` micro-batches; micro-batch k of the call takes the k mod A-th of the A
    frames in the rotation, in order of first annotation.  A micro-batch is one ``augment.draw()`` and TWO ``augment_frame`` calls with that
    draw -- the frame with the labelled plane, then with the object plane (the second warp of the image is accepted waste) -- the label
    1 / 0 / -1 (object / other / void) and ``TrainLoop.micro_batch(..., void_labels=True)``.  The network keeps training from round to
    round: nothing resets it.  ``set_previous(masks)`` hands over the last prediction for ``prior_distance`` (``training_planes``)."""

    def __init__(self, net, optimizer, frames_u8, object_id=1, n_ave_grad=5, augment=None, prior_distance=0, loop=None):
        g.check_int("object_id", object_id, 1, UNLABELLED - 1, "scribble")
        g.check_int("n_ave_grad", n_ave_grad, 1, 2 ** 31 - 1, "scribble")
        g.check_int("prior_distance", prior_distance, 0, 2 * SQDIST_MAX_SIDE, "scribble")
        if augment is None:
            from .augment import DeviceAugment
            augment = DeviceAugment(rots=(-30, 30), scales=(.75, 1.25))
        self.net, self.frames_u8, self.object_id, self.n_ave_grad, self.augment = net, frames_u8, int(object_id), int(n_ave_grad), augment
        self.prior_distance = int(prior_distance)
        self.loop = loop if loop is not None else TrainLoop(net, optimizer, mode='online', n_ave_grad=n_ave_grad)
        self.maps = {}            # frame -> merged uint8 [H,W] map, in order of first annotation
        self.two_class = {}       # frame -> its merged labels hold both classes
        self.previous = None      # the last prediction's masks, frame -> [H,W]
        self.micro_batches = 0

    def add(self, frame, scribble_map):
        frame = int(frame)
        if not 0 <= frame < len(self.frames_u8):
            raise ValueError("scribble: frame %d of a sequence of %d" % (frame, len(self.frames_u8)))
        if not isinstance(scribble_map, torch.Tensor) or scribble_map.dtype != torch.uint8 or scribble_map.dim() != 2:
            raise ValueError("scribble: a map is a uint8 [H,W] tensor")
        if tuple(scribble_map.shape) != tuple(self.frames_u8[frame].shape[:2]):
            raise ValueError("scribble: a map of %s for a frame of %s" % (tuple(scribble_map.shape), tuple(self.frames_u8[frame].shape[:2])))
        merged = merge_labels(self.maps.get(frame), scribble_map)
        self.maps[frame] = merged
        is_obj = merged == self.object_id
        both = torch.stack([is_obj.any(), ((merged != UNLABELLED) & ~is_obj).any()]).cpu()      # the read-back of this interaction
        self.two_class[frame] = bool(both[0]) and bool(both[1])
        return self.two_class[frame]

    def set_previous(self, masks):
        self.previous = masks

    @property
    def rotation(self):
        return [f for f in self.maps if self.two_class[f]]

    def labelled_pixels(self):
        """the labelled pixels of all merged maps (one read-back)"""
        if not self.maps:
            return 0
        return int(torch.stack([(m != UNLABELLED).sum() for m in self.maps.values()]).sum().item())

    def sample(self, frame):
        """one training sample of ``frame``: (image [1,3,H,W], label [1,1,H,W] in 1 / 0 / -1) under one draw of the augmentation"""
        prev = None if self.previous is None or not self.prior_distance else self.previous[frame]
        labelled, obj = training_planes(self.maps[frame], self.object_id, prev, self.prior_distance)
        flip, rot, sc = self.augment.draw()
        meanval = getattr(self.augment, 'meanval', MEANVAL)
        image, lab = augment_frame(self.frames_u8[frame], labelled, flip, rot, sc, meanval)
        _, obj = augment_frame(self.frames_u8[frame], obj, flip, rot, sc, meanval)
        label = torch.where(lab >= 0.5, (obj >= 0.5).to(lab.dtype), torch.full_like(lab, -1.0))
        return image[None], label[None]

    def fit(self, steps):
        """-> the micro-batches run: steps * n_ave_grad, or 0 when no frame holds both classes"""
        g.check_int("steps", steps, 0, 2 ** 31 - 1, "scribble")
        rotation = self.rotation
        if not rotation:
            return 0
        for k in range(steps * self.n_ave_grad):
            image, label = self.sample(rotation[k % len(rotation)])
            self.loop.micro_batch(image.detach().requires_grad_(), label, void_labels=True)
        self.micro_batches += steps * self.n_ave_grad
        return steps * self.n_ave_grad

    def image(self, frame):
        """the network's input of a frame, [1,3,H,W]: the identity pass of the augmentation kernel (mean subtracted, CHW)"""
        return augment_frame(self.frames_u8[frame], None, False, None, meanval=getattr(self.augment, 'meanval', MEANVAL))[0][None]

    def summary(self):
        return {"annotated": len(self.maps), "training": len(self.rotation), "left_out": len(self.maps) - len(self.rotation),
                "micro_batches": self.micro_batches}
