"""Stand-in engines for the host tests of the runner's output step (TEST INFRASTRUCTURE): one that must not be asked for anything,
and ``FakeEngine`` answered by the numpy twins with every call recorded.  numpy and the package alone: nothing here needs pytest or
a GPU."""
import numpy as np

from padel_analytics_amd import engine as E, heatmap as HM, mjpeg, render as R, topdown as T, video
from tests.fake_engine import FakeEngine


class StandInEngine:
    """An engine that must not be asked for anything: what is checked with it is decided before the output step touches one, or
    comes from the stored results alone."""

    def __getattr__(self, name):
        raise AssertionError(f"the engine was asked for {name}")


class TwinEngine(FakeEngine):
    """``FakeEngine`` plus ``warp``, ``heat``, ``render`` and ``jpeg_encode`` answered by the numpy twins on the stand-in buffers; every
    call is recorded in ``calls`` as (name, sizes, keyword arguments)."""

    def __init__(self):
        super().__init__(0)
        self.calls = []

    def record(self, name, sizes, kw) -> None:
        self.calls.append((name, sizes, kw))

    def warp(self, src, n, h, w, matrices, valid, dst, oh, ow, fill=(0, 0, 0)):
        self.record("warp", (n, h, w, oh, ow), dict(fill=tuple(fill)))
        frames = src.arr[:n * h * w * 3].reshape(n, h, w, 3)
        dst.arr[:n * oh * ow * 3] = T.warp_host(frames, matrices, valid, oh, ow, fill).reshape(-1)

    def heat(self, canvas, n, oh, ow, state, planes, points, first, valid, **call):
        self.record("heat", (n, oh, ow, planes), dict(call, points=np.array(points).reshape(-1, 3).tolist()))
        HM.accumulate_host(canvas.arr[:n * oh * ow * 3].reshape(n, oh, ow, 3), state.arr[:planes * oh * ow * 4].view(np.uint32).reshape(planes, oh, ow),
                           points, first, valid, **call)

    def render(self, src, n, h, w, marks, first, dst, **kw):
        self.record("render", (n, h, w), dict(kw))
        frames = src.arr[:n * h * w * 3].reshape(n, h, w, 3)
        got = R.render_host(frames, marks, first, kw.get("out", E.RENDER_BGR), kw.get("geom"), kw.get("enc"), scale=kw.get("scale", 1)).reshape(-1)
        dst.arr[:got.size] = got

    def jpeg_encode(self, buffer, n, h, w, desc, quality=90, out=None):
        self.record("jpeg_encode", (n, h, w), dict(quality=quality))
        return mjpeg.encode_host(buffer.arr[:video.yuv_span(n, h, w, desc)], n, h, w, desc, quality)


class FlatTwinEngine(TwinEngine):
    """``TwinEngine`` recording the way test_topdown_host.py reads it: ("warp", n, h, w, oh, ow, fill) and ("render", n, h, w)."""

    def record(self, name, sizes, kw) -> None:
        self.calls.append((name, *sizes, *([kw["fill"]] if name == "warp" else [])))
