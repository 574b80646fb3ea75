"""Seeded synthetic checkpoint of the court-keypoint ResNet-50 (there are no real weights offline), in the spirit of
oracle/synth_weights.py: He-initialised convolutions, BatchNorm running statistics CALIBRATED on the clip in float64 (every
BatchNorm sees zero-mean, unit-variance inputs on these frames, so no layer dies or blows up), and an ``fc`` scaled on the clip
so that the 24 logits of every frame are spread over the sigmoid's sensitive range.  A saturated or constant sigmoid would hide
any error behind it: tests/test_resnet_host.py asserts the two conditions (all logits in [-4, 4], standard deviation >= 0.3).
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests import resnet_ref as R
from tests import synth

FRAME_HW = (720, 1280)
N_FRAMES = 5


def test_frames(n: int = N_FRAMES, seed: int = 11) -> np.ndarray:
    return np.ascontiguousarray(synth.synthetic_frames(n, FRAME_HW[0], FRAME_HW[1], seed=seed))


class _Calibrator(R.ResNet50Ref):
    """Walks the network like the oracle, setting each BatchNorm's running statistics from the data it sees first."""

    def __init__(self, sd):
        super().__init__(sd, torch.float64)
        self.stats = {}

    def _conv(self, x, name, stride, pad):
        y = super()._conv(x, name, stride, pad)
        bn = {"conv1": "bn1"}.get(name) or (name.replace("downsample.0", "downsample.1") if "downsample" in name
                                            else name.replace(".conv", ".bn"))
        mu = y.mean(dim=(0, 2, 3)).float()
        var = y.var(dim=(0, 2, 3), unbiased=False).clamp_min(1e-4).float()
        self.stats[f"{bn}.running_mean"], self.stats[f"{bn}.running_var"] = mu.numpy(), var.numpy()
        self.sd[f"{bn}.running_mean"], self.sd[f"{bn}.running_var"] = mu.double(), var.double()
        return y


@torch.no_grad()
def synthetic_state_dict(frames_bgr, seed: int = 0, n_out: int = 24) -> dict:
    rng = np.random.default_rng(seed)
    sd = {}
    for k, shape in R.state_dict_shapes(n_out).items():
        if k.endswith("conv1.weight") or k.endswith("conv2.weight") or k.endswith("conv3.weight") or k.endswith("downsample.0.weight"):
            fan_in = shape[1] * shape[2] * shape[3]
            sd[k] = rng.normal(0.0, (2.0 / fan_in) ** 0.5, shape).astype(np.float32)
        elif k.endswith("running_mean"):
            sd[k] = np.zeros(shape, np.float32)
        elif k.endswith("running_var"):
            sd[k] = np.ones(shape, np.float32)
        elif k.endswith("bn3.weight"):
            sd[k] = rng.uniform(0.3, 0.7, shape).astype(np.float32)       # the residual branch enters the join at half weight
        elif ".bn" in k or k.startswith("bn1") or "downsample.1" in k:
            sd[k] = (rng.uniform(0.7, 1.3, shape) if k.endswith("weight") else rng.normal(0.0, 0.2, shape)).astype(np.float32)
        elif k == "fc.weight":
            sd[k] = rng.normal(0.0, 1.0, shape).astype(np.float32)
        else:
            sd[k] = np.zeros(shape, np.float32)
    cal = _Calibrator(sd)
    x = R.preprocess(frames_bgr)
    feat = torch.flatten(F.adaptive_avg_pool2d(cal.features(x), 1), 1).numpy()            # (n, 2048) float64
    sd.update(cal.stats)
    # fc: the part of a logit that changes from frame to frame gets an RMS of 0.6, its mean over the clip a seeded offset in
    # [-1.8, 1.8] — every logit of the clip then lies well inside [-4, 4] and the set is far from constant
    z = feat @ sd["fc.weight"].astype(np.float64).T
    dev = z - z.mean(axis=0, keepdims=True)
    scale = 0.6 / max(float(np.sqrt((dev ** 2).mean())), 1e-12)
    w = (sd["fc.weight"].astype(np.float64) * scale).astype(np.float32)
    offsets = rng.uniform(-1.8, 1.8, n_out)
    sd["fc.weight"] = w
    sd["fc.bias"] = (offsets - (feat @ w.astype(np.float64).T).mean(axis=0)).astype(np.float32)
    return sd


@functools.lru_cache(maxsize=2)
def clip_and_state_dict(seed: int = 0):
    """(frames (5, 720, 1280, 3) uint8 BGR, state_dict) — cached: the calibration pass is a float64 ResNet-50 forward."""
    frames = test_frames()
    return frames, synthetic_state_dict(frames, seed)


def save_plain(path, sd) -> None:
    """``torch.save(model.state_dict())``: the file format the reference loads (keypoints_tracker.py:165)."""
    from collections import OrderedDict
    torch.save(OrderedDict((k, torch.from_numpy(np.ascontiguousarray(v))) for k, v in sd.items()), str(path))
