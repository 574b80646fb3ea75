"""CPU oracle of the court-keypoint regressor: a restatement, in plain torch functional calls, of what the reference's
``KeypointsTracker(model_type="resnet")`` computes (``trackers/keypoints_tracker/keypoints_tracker.py:158-168, 286-289``;
preprocessing ``iterable.py:10-39``): BGR -> RGB, ``transforms.Resize((224, 224))`` on a PIL image (Pillow BILINEAR),
``ToTensor``, ``Normalize``, torchvision's ResNet-50 (v1.5: the stride of a stage sits on ``conv2`` of its first bottleneck,
BatchNorm in eval mode, eps 1e-5) with a 24-way ``fc``, sigmoid.

torchvision is not installed here, so this file is NOT pinned against it by running both: it is pinned by known answers
(tests/test_resnet_host.py) — the published parameter count 25,557,032 with a 1000-way ``fc``, the published 4.09 G
multiply-accumulates at 224 x 224, and the exact key / shape set of a torchvision ``state_dict``.  ``dtype`` selects the
arithmetic: float32 is what the reference runs, float64 is the yardstick both are measured against.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

LAYERS = (3, 4, 6, 3)
EXPANSION = 4
INPUT = 224
BN_EPS = 1e-5
# the reference's Normalize: the green mean is 0.465 there (iterable.py:21), not ImageNet's 0.456
MEAN = (0.485, 0.465, 0.406)
STD = (0.229, 0.224, 0.225)
BN_KEYS = ("weight", "bias", "running_mean", "running_var")


def blocks():
    """[(prefix, cin, planes, stride, has_downsample)] of the 16 bottlenecks in forward order."""
    out, cin = [], 64
    for n, count in enumerate(LAYERS, 1):
        planes = 64 * 2 ** (n - 1)
        for i in range(count):
            out.append((f"layer{n}.{i}", cin, planes, 2 if (i == 0 and n > 1) else 1, i == 0))
            cin = planes * EXPANSION
    return out


def convs(n_out: int = 24):
    """[(weight key, bn prefix | None, cout, cin, k, stride, level of the output map)] of every conv in forward order (level l:
    a map of 224 >> l pixels per side)."""
    out = [("conv1", "bn1", 64, 3, 7, 2, 1)]
    level = 2
    for p, cin, planes, stride, down in blocks():
        lout = level + (stride == 2)
        out.append((f"{p}.conv1", f"{p}.bn1", planes, cin, 1, 1, level))
        out.append((f"{p}.conv2", f"{p}.bn2", planes, planes, 3, stride, lout))
        out.append((f"{p}.conv3", f"{p}.bn3", planes * EXPANSION, planes, 1, 1, lout))
        if down:
            out.append((f"{p}.downsample.0", f"{p}.downsample.1", planes * EXPANSION, cin, 1, stride, lout))
        level = lout
    return out


def state_dict_shapes(n_out: int = 24) -> dict:
    sh = {}
    for name, bn, cout, cin, k, _, _ in convs(n_out):
        sh[f"{name}.weight"] = (cout, cin, k, k)
        for key in BN_KEYS:
            sh[f"{bn}.{key}"] = (cout,)
    sh["fc.weight"] = (n_out, 512 * EXPANSION)
    sh["fc.bias"] = (n_out,)
    return sh


def count_params(n_out: int = 24) -> int:
    """Learnable parameters (BatchNorm running statistics are buffers)."""
    return sum(int(np.prod(s)) for k, s in state_dict_shapes(n_out).items() if "running_" not in k)


def macs(n_out: int = 1000, size: int = INPUT) -> int:
    """Multiply-accumulates of the convolutions and the linear layer for one size x size image."""
    total = 0
    for _, _, cout, cin, k, _, level in convs(n_out):
        total += (size >> level) ** 2 * cout * cin * k * k
    return total + n_out * 512 * EXPANSION


def norm_table() -> np.ndarray:
    """[3][256] float32: ToTensor (``/ 255``) then Normalize (``- mean``, ``/ std``), all in float32."""
    b = np.arange(256).astype(np.float32) / np.float32(255.0)
    return np.stack([((b - np.float32(MEAN[c])) / np.float32(STD[c])) for c in range(3)])


def resize_rgb_u8(frame_bgr: np.ndarray) -> np.ndarray:
    """(h, w, 3) uint8 BGR -> (224, 224, 3) uint8 RGB through Pillow itself."""
    from PIL import Image
    rgb = np.ascontiguousarray(frame_bgr[..., ::-1])
    return np.asarray(Image.fromarray(rgb).resize((INPUT, INPUT), Image.BILINEAR))


def preprocess(frames_bgr) -> torch.Tensor:
    """-> (n, 3, 224, 224) float32, exactly the reference's tensor."""
    out = []
    for f in frames_bgr:
        x = torch.from_numpy(resize_rgb_u8(f).copy()).permute(2, 0, 1).to(torch.float32).div(255)
        mean = torch.as_tensor(MEAN, dtype=torch.float32)[:, None, None]
        std = torch.as_tensor(STD, dtype=torch.float32)[:, None, None]
        out.append(x.sub_(mean).div_(std))
    return torch.stack(out)


class ResNet50Ref:
    def __init__(self, sd, dtype=torch.float32):
        self.dtype = dtype
        self.sd = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items() if not k.endswith("num_batches_tracked")}

    def _bn(self, x, p):
        return F.batch_norm(x, self.sd[f"{p}.running_mean"], self.sd[f"{p}.running_var"], self.sd[f"{p}.weight"], self.sd[f"{p}.bias"],
                            False, 0.0, BN_EPS)

    def _conv(self, x, name, stride, pad):
        return F.conv2d(x, self.sd[f"{name}.weight"], None, stride=stride, padding=pad)

    def stem(self, x):
        return F.relu(self._bn(self._conv(x.to(self.dtype), "conv1", 2, 3), "bn1"))

    def features(self, x):
        """-> the (n, 2048, 7, 7) map behind layer4."""
        x = F.max_pool2d(self.stem(x), 3, 2, 1)
        for p, _, _, stride, down in blocks():
            idt = x
            y = F.relu(self._bn(self._conv(x, f"{p}.conv1", 1, 0), f"{p}.bn1"))
            y = F.relu(self._bn(self._conv(y, f"{p}.conv2", stride, 1), f"{p}.bn2"))
            y = self._bn(self._conv(y, f"{p}.conv3", 1, 0), f"{p}.bn3")
            if down:
                idt = self._bn(self._conv(x, f"{p}.downsample.0", stride, 0), f"{p}.downsample.1")
            x = F.relu(y + idt)
        return x

    @torch.no_grad()
    def logits(self, x):
        f = torch.flatten(F.adaptive_avg_pool2d(self.features(x), 1), 1)
        return F.linear(f, self.sd["fc.weight"], self.sd["fc.bias"])


@torch.no_grad()
def predict(sd, frames_bgr, dtype=torch.float32):
    """-> (xy (n, 24) sigmoid outputs, logits (n, 24)) as numpy arrays of ``dtype``."""
    z = ResNet50Ref(sd, dtype).logits(preprocess(frames_bgr))
    return torch.sigmoid(z).numpy(), z.numpy()


def keypoints_px(xy: np.ndarray, w_frame: int, h_frame: int) -> np.ndarray:
    """(n, 24) fractions -> (n, 12, 2) pixels."""
    return np.asarray(xy, np.float64).reshape(len(xy), 12, 2) * np.array([w_frame, h_frame], np.float64)
