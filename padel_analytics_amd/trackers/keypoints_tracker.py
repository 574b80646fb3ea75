"""Court keypoints tracker — drop-in for the reference's ``trackers/keypoints_tracker/keypoints_tracker.py``
(``Keypoint`` :17-66, ``Keypoints`` :69-117, ``KeypointsTracker`` :122-312), SURVEY.md §8(f)#4.

In the shipped configuration the reference never runs a model here: ``main.py:81-104,154-161`` always passes
``fixed_keypoints_detection`` and both predict methods short-circuit (:204-209, :266-271).  The "yolo" model
type (:199-262) is just another YOLOv8-pose graph (K = 12 keypoints, ``max_det = 12``, conf .5, Pillow stretch
to 640x640) and runs on the same HIP engine as the players keypoints tracker.  The "resnet" type — the constructor's
default: a torchvision ResNet-50 whose 24 sigmoid outputs are the 12 keypoints as fractions of the frame (:158-168, :273-312,
preprocessing ``iterable.py:10-39``) — runs on the engine too (``resnet.CourtResNet``: BGR -> RGB, Pillow bilinear resize to
224 x 224, normalisation, network, sigmoid on the device); it consumes the frame stream in ``predict_frames`` in batches of
``batch_size`` and its ``predict_sample`` raises ``NoPredictSample``, as in the reference.  Construction opens no file: the
checkpoint is resolved by ``to`` / at the top of ``predict_frames``, where a file that is missing, unreadable or not a
ResNet-50 with a 24-way ``fc`` raises ``NotImplementedError`` ("no court model this engine can run") chained from the cause.
"""
from __future__ import annotations

from pathlib import Path
from typing import Iterable, Optional, Type

import numpy as np

from .. import video
from .tracker import NoPredictFrames, NoPredictSample, Object, Tracker, _sampler


class Keypoint:
    def __init__(self, id: int, xy: tuple):
        self.id = id
        self.xy = xy

    @classmethod
    def from_json(cls, x: dict): return cls(**x)

    def serialize(self) -> dict: return {"id": self.id, "xy": self.xy}

    def asint(self) -> tuple: return tuple(int(v) for v in self.xy)

    def marks(self) -> list:
        """Reference :45-70: ``str(id + 1)`` in white with its bottom-left at (x + 5, y - 5) — here the renderer's 5 x 7 font at
        scale 1 — then a filled circle of radius 6 in RGB (255, 0, 0)."""
        from .. import render
        x, y = self.asint()
        return render.text(str(self.id + 1), x + 5, y - 5 - (render.GLYPH_H - 1), 1, (255, 255, 255)) + [render.disc(x, y, 6, (0, 0, 255))]


class Keypoints(Object):
    def __init__(self, keypoints: list):
        super().__init__()
        self.keypoints = sorted(keypoints, key=lambda k: k.id)
        self.keypoints_by_id = {k.id: k for k in keypoints}

    @classmethod
    def from_json(cls, x: list) -> "Keypoints":
        return cls([Keypoint.from_json(k) for k in x])

    def serialize(self) -> list: return [k.serialize() for k in self.keypoints]

    def __len__(self) -> int: return len(self.keypoints)

    def __iter__(self): return iter(self.keypoints)

    def __getitem__(self, id: int) -> Keypoint: return self.keypoints_by_id[id]

    def marks(self, **kwargs) -> list:
        return [m for k in self.keypoints for m in k.marks()]


class KeypointsTracker(Tracker):
    NUMBER_KEYPOINTS = 12
    TRAIN_IMAGE_SIZE = 640
    CONF = 0.5
    IOU = 0.7
    # model output index -> court keypoint id (reference :215-228)
    POINTS_MAPPER = {0: 10, 1: 11, 2: 1, 3: 0, 4: 7, 5: 9, 6: 8, 7: 5, 8: 6, 9: 2, 10: 4, 11: 3}

    def __init__(self, model_path: str, batch_size: int, model_type: str = "resnet",
                 fixed_keypoints_detection: Optional[Keypoints] = None,
                 load_path: Optional[str | Path] = None, save_path: Optional[str | Path] = None):
        super().__init__(load_path=load_path, save_path=save_path)
        if model_type not in ("resnet", "yolo"):
            raise ValueError("Unknown model type")
        self.batch_size = batch_size
        self.model_type = model_type
        self.model_path = model_path
        self.fixed_keypoints_detection = fixed_keypoints_detection
        self._model = None

    @property
    def model(self):
        if self._model is None:
            if self.model_type == "yolo":
                from ..yolo import YOLO
                self._model = YOLO(self.model_path)
            else:
                from ..resnet import CourtResNet
                try:
                    self._model = CourtResNet(self.model_path)
                except (OSError, ValueError) as err:      # missing / unreadable file, not a ResNet-50 with a 24-way fc
                    raise NotImplementedError(f"{self.model_path}: no court model this engine can run ({err})") from err
        return self._model

    @property
    def streams(self):
        """The ResNet regressor consumes the stream in ``predict_frames`` (runner: no probing call, no file opened for it)."""
        return True if (self.model_type == "resnet" and self.fixed_keypoints_detection is None) else None

    def video_info_post_init(self, video_info) -> "KeypointsTracker": return self

    def object(self) -> Type[Object]: return Keypoints

    def draw_kwargs(self) -> dict: return {}

    def __str__(self) -> str: return "keypoints_tracker"

    def restart(self) -> None: self.results.restart()

    def to(self, device: str) -> None:
        if self.fixed_keypoints_detection is None:
            self.model.to(device)

    def predict_sample(self, sample: Iterable[np.ndarray], **kwargs) -> list:
        sample = list(sample)
        if self.fixed_keypoints_detection is not None:
            print(f"{self.__str__()}: using fixed court keypoints")
            return [self.fixed_keypoints_detection for _ in sample]
        if self.model_type != "yolo":
            raise NoPredictSample()
        h_frame, w_frame = sample[0].shape[:2]
        ratio_x, ratio_y = w_frame / self.TRAIN_IMAGE_SIZE, h_frame / self.TRAIN_IMAGE_SIZE
        results = self.model.predict_frames(sample, self.CONF, self.IOU, self.TRAIN_IMAGE_SIZE, classes=None,
                                            max_det=self.NUMBER_KEYPOINTS, channel_reverse=True, pil_stretch=True)
        predictions = []
        for result in results:
            xy = result.keypoints.xy
            kps = []
            if len(xy):                                   # the reference assumes exactly one court detection
                for i, kp in enumerate(xy[0]):
                    kps.append(Keypoint(id=self.POINTS_MAPPER.get(i, i), xy=(float(kp[0]) * ratio_x, float(kp[1]) * ratio_y)))
            predictions.append(Keypoints(kps))
        return predictions

    def predict_frames(self, frame_generator: Iterable[np.ndarray], **kwargs) -> list:
        if self.fixed_keypoints_detection is not None:
            print(f"{self.__str__()}: using fixed court keypoints")
            return [self.fixed_keypoints_detection for _ in frame_generator]
        if self.model_type == "yolo":
            raise NoPredictFrames()
        model = self.model                    # resolved before the generator is touched: an unusable checkpoint fails here
        model.set_max_batch(self.batch_size)
        predictions = []
        for sample in _sampler(iter(frame_generator), self.batch_size):      # (an empty generator yields no batch)
            dev = video.device_batch(sample)
            if dev is not None:
                buf, n, h_frame, w_frame = dev
                outputs = model.infer(buf, n, h_frame, w_frame)
            else:
                frames = video.host_batch(sample)
                h_frame, w_frame = frames.shape[1:3]
                outputs = model.infer(frames)
            predictions.extend(self.keypoints_from_outputs(outputs, w_frame, h_frame))
        return predictions

    @classmethod
    def keypoints_from_outputs(cls, outputs: np.ndarray, w_frame: int, h_frame: int) -> list:
        """(n, 24) float32 sigmoid outputs -> ``Keypoints`` per frame: ids 0..11 (``POINTS_MAPPER`` is the YOLO model's), xy =
        (out[2i] * w_frame, out[2i + 1] * h_frame) as numpy computes float32 x int in the reference (:296-300)."""
        out = []
        for row in np.asarray(outputs, np.float32):
            out.append(Keypoints([Keypoint(i, (float(kp[0] * w_frame), float(kp[1] * h_frame)))      # (the float32 product, as a JSON-able float)
                                  for i, kp in enumerate(row.reshape(cls.NUMBER_KEYPOINTS, 2))]))
        return out
