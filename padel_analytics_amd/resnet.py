"""``CourtResNet`` — the court-keypoint regressor of the reference's ``KeypointsTracker(model_type="resnet")``
(``trackers/keypoints_tracker/keypoints_tracker.py:158-168, 286-289``): a torchvision ResNet-50 whose ``fc`` has 24 outputs
(12 keypoints x (x, y) as fractions of the frame), behind a sigmoid.

The file is a bare ``torch.save(model.state_dict())``.  Everything numeric — BGR -> RGB, Pillow's bilinear resize to 224 x 224,
normalisation, the 53 convolutions, pooling, ``fc`` and the sigmoid — runs in ``libpadel_hip.so`` (``graph.build_resnet50``,
``pa_resnet_infer``); this file only loads, places and marshals.  Arithmetic as for the other graphs: fp16 pairs ("h2") by
default, repeated on the full-range bf16x3 kernels when an activation leaves the fp16 range.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import checkpoint, engine as E, graph as G


class CourtResNet:
    OUTPUTS = G.RESNET_OUT

    def __init__(self, model_path=None, engine: Optional[E.Engine] = None, fp32_mode: Optional[str] = None, *, state_dict=None):
        """Raises ``FileNotFoundError`` / ``OSError`` for a file that cannot be read and ``ValueError`` for one that is not a
        torchvision ResNet-50 with a 24-way ``fc``.  Touches no device: ``to("cuda")`` / the first ``infer`` does."""
        sd = state_dict if state_dict is not None else checkpoint.load_state_dict(model_path)
        G.check_resnet50_state_dict(sd)
        self.state_dict = sd
        self.fp32_mode = fp32_mode or E.fp32_mode()
        self._engine = engine
        self._model: Optional[E.Model] = None
        self.max_batch = 64
        self.fell_back = False           # an h2 model overflowed: this object runs on the bx3 kernels from then on

    def _ensure_model(self) -> E.Model:
        if self._model is None:
            graph = G.build_resnet50(self.state_dict, dtype=E.graph_dtype(self.fp32_mode))
            self._model = E.Model(self._engine or E.default_engine(), graph)
            self._model.set_max_batch(self.max_batch)
        return self._model

    def set_fp32_mode(self, mode: str) -> None:
        """"h2" | "bx3" (as ``yolo.YOLO.set_fp32_mode``): the HBM model is rebuilt on next use.  A sharded run switches every
        rank at once through this (``Tracker.use_full_range``) when one of them overflowed."""
        if mode not in ("h2", "bx3"):
            raise ValueError(mode)
        if mode != self.fp32_mode:
            self.fp32_mode = mode
            self.close()

    def to(self, device) -> "CourtResNet":
        dev = str(device)
        if dev.startswith("cuda") or dev.isdigit():
            self._ensure_model()
        elif dev == "cpu":
            import os
            if os.environ.get("PADEL_RELEASE_ON_CPU") == "1":       # as yolo.YOLO.to: the weights stay resident by default
                self.close()
        else:
            raise ValueError(f"unknown device {device!r}")
        return self

    def set_max_batch(self, n: int) -> None:
        self.max_batch = int(n)
        if self._model is not None:
            self._model.set_max_batch(self.max_batch)

    def close(self) -> None:
        if self._model is not None:
            self._model.close()
            self._model = None

    def infer(self, frames, n: Optional[int] = None, h: Optional[int] = None, w: Optional[int] = None, *, want_logits: bool = False):
        """frames: (n, h, w, 3) uint8 BGR video frames (ndarray, or an ``engine.DeviceBuffer`` with n, h, w given) ->
        xy (n, 24) float32 in [0, 1] (and the logits with ``want_logits``)."""
        if not isinstance(frames, E.DeviceBuffer):
            frames = np.ascontiguousarray(frames, np.uint8)
            n, h, w = frames.shape[:3]
        m = self._ensure_model()
        xy, logits = m.resnet_infer(frames, n, h, w, want_logits=want_logits)
        if self.fp32_mode == "h2" and m.take_overflow():
            self.close()
            self.fp32_mode, self.fell_back = "bx3", True
            xy, logits = self._ensure_model().resnet_infer(frames, n, h, w, want_logits=want_logits)
        return (xy, logits) if want_logits else xy
