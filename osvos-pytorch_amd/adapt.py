"""Online adaptation over the sequence (OnAVOS-style) on top of the fast fine-tune: after the first-frame fine-tuning, every later frame
gets a few optimizer steps of its own before it is segmented.  The targets of those steps come from the network's own confident output and
from the previous frame's mask, made on the device by ``osvos_adapt_targets`` (csrc/distance.hip):

  * negative (0): farther than ``distance`` pixels from the previous frame's mask eroded by ``erosion`` pixels
  * positive (1): not negative, and the fused logit above ``log(prob / (1 - prob))``
  * void (-1): everything else -- ignored by the class-balanced loss (``void_labels`` / OSVOS_CBCE_VOID)

and the steps on the current frame are interleaved with steps on the annotated first frame, so the network does not drift.  Everything is
enqueued; the only read-back is the 24 bytes of class counts per frame that decide whether the frame is usable at all."""
import numpy as np
import torch

from . import _glue as g
from ._lib import lib
from .results import mask_bytes_nhw
from .train_common import TrainLoop


def adaptation_targets(logits, prev_mask, prob=0.97, erosion=15, distance=220):
    """logits: float32 CUDA tensor [N,1,H,W] or [N,H,W] (the fused output), prev_mask: the previous frame's final mask (uint8, bool or float;
    [N,1,H,W], [N,H,W] or [H,W]; non-zero = object) -> ``(label, counts)``: label float32 [N,1,H,W] with 1 / 0 / -1 = positive / negative /
    void, counts int64 [N,3] = (n_pos, n_neg, n_void), both on the device.  Enqueued only."""
    g.need_cuda(logits, "logits", "adapt")
    if not 0.0 < prob < 1.0:
        raise ValueError("prob must be a probability in (0, 1), got %r" % (prob,))
    if int(erosion) < 0 or int(distance) < 0:
        raise ValueError("erosion and distance are pixel counts >= 0, got %r and %r" % (erosion, distance))
    m, n, h, w = mask_bytes_nhw(prev_mask, "adaptation_targets", "adapt")
    x = logits.detach().float().contiguous()
    if x.numel() != n * h * w or tuple(x.shape[-2:]) != (h, w) or x.device != m.device:
        raise ValueError("logits of shape %r next to a mask of %d frames of %d x %d" % (tuple(logits.shape), n, h, w))
    label = torch.empty((n, 1, h, w), device=x.device, dtype=torch.float32)
    counts = torch.empty((n, 3), device=x.device, dtype=torch.int64)
    ws = g.workspace(lib().osvos_adapt_ws_bytes(n, h, w), x.device, what="%d frames of %d x %d" % (n, h, w), prefix="adapt", dtype=torch.int32)
    g.call("adapt_targets", x.device, g.ptr(x), g.ptr(m), float(np.log(prob / (1.0 - prob))), int(erosion), int(distance), g.ptr(label), g.ptr(counts),
           n, h, w, g.ptr(ws))
    return label, counts


def first_frame_source(loader):
    """``first_inputs`` of ``OnlineAdapter`` from a loader whose passes yield {'image', 'gt'} samples of the annotated frame, freshly
    augmented on every pass (train_online.DeviceTrainFrame)."""
    def draw():
        s = next(iter(loader))
        return s['image'], s['gt']
    return draw


class OnlineAdapter(object):
    """``adapter(image, prev_mask)`` -> the fused logits [N,1,H,W] of ``image`` after adapting the network on it:

      1. one forward without gradients, and the targets from its fused logits and ``prev_mask``;
      2. ``steps`` optimizer steps: step k (0-based) trains on ``image`` against the targets (void labels, gradient times ``weight``) when
         ``k % mix == mix - 1``, and otherwise on a fresh ``first_inputs()`` -- (image, gt) of the annotated first frame -- against its
         annotation;
      3. one more forward without gradients, which is returned.

    A frame whose targets hold no positive or no negative pixel is skipped: only its first-frame steps run.  ``steps = 0`` is one plain
    forward and nothing else.  The adapter owns a ``TrainLoop`` with one micro-batch per optimizer step; it turns gradients on for its
    training steps itself, so it can be called under ``torch.no_grad()``."""

    def __init__(self, net, optimizer, first_inputs, steps=15, mix=5, weight=1.0, prob=0.97, erosion=15, distance=220):
        if int(steps) < 0 or int(mix) < 1:
            raise ValueError("steps >= 0 and mix >= 1, got %r and %r" % (steps, mix))
        if not 0.0 < prob < 1.0:
            raise ValueError("prob must be a probability in (0, 1), got %r" % (prob,))
        if int(erosion) < 0 or int(distance) < 0:
            raise ValueError("erosion and distance are pixel counts >= 0, got %r and %r" % (erosion, distance))
        if not callable(first_inputs):
            raise ValueError("first_inputs must be a callable that returns (image, gt) of the annotated frame")
        self.net, self.first_inputs = net, first_inputs
        self.steps, self.mix, self.weight = int(steps), int(mix), float(weight)
        self.prob, self.erosion, self.distance = float(prob), int(erosion), int(distance)
        self.loop = TrainLoop(net, optimizer, mode='online', n_ave_grad=1)
        self.forward = None          # a callable image -> logit maps to use in place of net.forward for the two plain forwards (match.AppearanceMatcher)
        self.adapted = self.skipped = self.steps_taken = 0

    def _forward(self, image):
        with torch.no_grad():
            return (self.forward or self.net.forward)(image)[-1]

    def __call__(self, image, prev_mask):
        if self.steps == 0:
            return self._forward(image)
        dev = image.device
        label, counts = adaptation_targets(self._forward(image), prev_mask, self.prob, self.erosion, self.distance)
        n_pos, n_neg = (int(v) for v in counts[:, :2].sum(0).cpu().numpy())      # the one read-back of a frame
        usable = n_pos > 0 and n_neg > 0
        if usable:
            self.adapted += 1
        else:
            self.skipped += 1
        with torch.enable_grad():
            for k in range(self.steps):
                if k % self.mix == self.mix - 1:
                    if usable:
                        self.loop.micro_batch(image.detach(), label, void_labels=True, grad_scale=self.weight)
                        self.steps_taken += 1
                    continue
                first, gt = self.first_inputs()
                self.loop.micro_batch(first.to(dev).detach(), gt.to(dev))
                self.steps_taken += 1
        return self._forward(image)

    def summary(self):
        """{'adapted', 'skipped', 'steps'}: frames adapted on, frames skipped for want of a class, optimizer steps taken (host counters)."""
        return {"adapted": self.adapted, "skipped": self.skipped, "steps": self.steps_taken}
