"""``Engine.heat`` (csrc/heat.hip, ``pa_heat_accumulate``) on the GPU against its numpy twin ``heatmap.accumulate_host``, bit for bit in
canvases AND state, the store path asserted per case through ``Engine.heat_last_path``, sentinel bytes around both buffers: points
in the corners, on the edges, half and wholly outside, overlapping discs, r = 1 and r = 255, 1..4 planes with every ``show_mask`` of
two, 64 points in a frame and a batch with none, frames that are not valid, ``alpha`` 0 and 256, a state near saturation, the state
carried over two calls, canvases larger than one pass of the grid-stride loop, misaligned buffers, and every refusal — which
launches nothing."""
import numpy as np
import pytest

from padel_analytics_amd import engine as E
from tests import heat_cases as HC

pytestmark = pytest.mark.gpu

PAD = 64            # sentinel bytes kept in front of and behind the canvases and the state
NAMED = HC.named_cases()


class Device:
    """The canvases and the state of a case in HBM, each ``PAD + shift`` bytes into a buffer filled with 0x5A."""

    def __init__(self, eng, canvases, state, canvas_shift=0, state_shift=0):
        self.eng, self.cshape, self.sshape = eng, canvases.shape, state.shape
        self.c_at, self.s_at = PAD + canvas_shift, PAD + state_shift
        self.cbuf = eng.alloc(canvases.nbytes + 2 * PAD + canvas_shift)
        self.sbuf = eng.alloc(state.nbytes + 2 * PAD + state_shift)
        for buf, at, a in ((self.cbuf, self.c_at, canvases), (self.sbuf, self.s_at, state)):
            whole = np.full(buf.nbytes, 0x5A, np.uint8)
            whole[at:at + a.nbytes] = a.reshape(-1).view(np.uint8)
            buf.upload(whole)
        self.canvas = self.cbuf.view(self.c_at, canvases.nbytes)
        self.state = self.sbuf.view(self.s_at, state.nbytes)

    def heat(self, points, first, valid, **call) -> int:
        n, oh, ow = self.cshape[:3]
        self.eng.heat(self.canvas, n, oh, ow, self.state, self.sshape[0], points, first, valid, **call)
        return self.eng.heat_last_path()

    def read(self) -> tuple:
        """(canvases, state); the bytes on both sides of each must come back untouched."""
        out = []
        for buf, at, shape, dtype in ((self.cbuf, self.c_at, self.cshape, np.uint8), (self.sbuf, self.s_at, self.sshape, np.uint32)):
            whole = buf.download(np.empty(buf.nbytes, np.uint8))
            size = int(np.prod(shape)) * np.dtype(dtype).itemsize
            assert np.all(whole[:at] == 0x5A) and np.all(whole[at + size:] == 0x5A), "bytes around a buffer were written"
            out.append(whole[at:at + size].copy().view(dtype).reshape(shape))
        return tuple(out)

    def free(self):
        self.eng.synchronize()
        self.cbuf.free()
        self.sbuf.free()


def both(eng, c: HC.Case, want_path, canvas_shift=0, state_shift=0):
    want_canvases, want_state = HC.twin(c)
    dev = Device(eng, c.canvases, c.state, canvas_shift, state_shift)
    try:
        path = dev.heat(c.points, c.first, c.valid, **c.call)
        canvases, state = dev.read()
    finally:
        dev.free()
    assert path == want_path
    assert np.array_equal(state, want_state), f"{int((state != want_state).sum())} of {state.size} densities differ"
    differ = (canvases != want_canvases).any(axis=-1)
    assert not differ.any(), f"{int(differ.sum())} of {differ.size} pixels differ"
    return canvases, state


@pytest.mark.parametrize("name", list(NAMED))
def test_against_the_twin_on_both_store_paths(gpu_engine, name):
    c = NAMED[name]
    canvases, state = both(gpu_engine, c, E.HEAT_PATH_VECTOR if name.startswith("vector") else E.HEAT_PATH_BYTE)
    if "alpha 0" in name:                                     # the pixels stay, the state moves
        assert np.array_equal(canvases, c.canvases) and state.any()
    if "no point" in name:
        assert np.array_equal(state, c.state) and not np.array_equal(canvases, c.canvases)
    if "saturation" in name:
        assert int(state.max()) == 2 ** 32 - 1
    if "not valid" in name:
        assert np.array_equal(canvases[1], c.canvases[1]) and not np.array_equal(canvases, c.canvases)


@pytest.mark.parametrize("oh, ow, path", [(33, 50, E.HEAT_PATH_BYTE), (32, 48, E.HEAT_PATH_VECTOR)])
def test_the_state_is_carried_over_two_calls(gpu_engine, oh, ow, path):
    """One call of 6 frames against two calls of 3 on the same buffers: the same maps, the same canvases."""
    rng = np.random.default_rng(3)
    c = HC.make("carried", rng, 6, oh, ow, 3, HC.random_points(rng, 6, oh, ow, 3, 6), 6, full=900)
    want_canvases, want_state = HC.twin(c)
    dev = Device(gpu_engine, c.canvases, c.state)
    try:
        for lo in (0, 3):
            k0, k1 = int(c.first[lo]), int(c.first[lo + 3])              # frames lo .. lo + 3 of the same canvases, the same state
            n3 = 3 * oh * ow * 3
            gpu_engine.heat(dev.canvas.view(lo * oh * ow * 3, n3), 3, oh, ow, dev.state, 3, c.points[k0:k1], c.first[lo:lo + 4] - k0,
                            c.valid[lo:lo + 3], **c.call)
            assert gpu_engine.heat_last_path() == path
        canvases, state = dev.read()
    finally:
        dev.free()
    assert np.array_equal(state, want_state) and np.array_equal(canvases, want_canvases)


@pytest.mark.parametrize("oh, ow, path", [(760, 700, E.HEAT_PATH_BYTE), (2060, 4096, E.HEAT_PATH_VECTOR)])
def test_a_canvas_larger_than_one_pass_of_the_grid(gpu_engine, oh, ow, path):
    """A launch covers 2048 x 256 threads at once: 524 288 pixels on the byte path, 16 times as many on the 16-byte path.  760 x 700 =
    532 000 and 2060 x 4096 / 16 = 527 360 threads take a second pass of the loop; the points lie in the first and in the last rows."""
    assert oh * ow // (16 if path == E.HEAT_PATH_VECTOR else 1) > 2048 * 256
    rng = np.random.default_rng(5)
    c = HC.make("large", rng, 1, oh, ow, 1, [[(3, 2, 0), (ow - 5, oh - 2, 0), (ow // 2, oh - 1, 0)]], 40, full=400)
    canvases, state = both(gpu_engine, c, path)
    assert state[0, oh - 1, ow // 2] == 255 and state[0, 2, 3] == 255


def test_misaligned_buffers_take_the_byte_path(gpu_engine):
    c = NAMED["vector: corners, edges, outside, overlapping"]     # 48 columns would allow 16-byte accesses: the addresses do not
    for shift in (1, 4, 15):
        both(gpu_engine, c, E.HEAT_PATH_BYTE, canvas_shift=shift)
    both(gpu_engine, c, E.HEAT_PATH_BYTE, state_shift=4)
    both(gpu_engine, c, E.HEAT_PATH_BYTE, canvas_shift=3, state_shift=8)
    both(gpu_engine, c, E.HEAT_PATH_VECTOR, canvas_shift=16, state_shift=32)


def test_a_width_of_16_k_plus_1_and_one_pixel(gpu_engine):
    rng = np.random.default_rng(9)
    both(gpu_engine, HC.make("65", rng, 3, 7, 65, 2, HC.random_points(rng, 3, 7, 65, 2, 4), 4), E.HEAT_PATH_BYTE)
    both(gpu_engine, HC.make("1", rng, 3, 1, 1, 1, [[(0, 0, 0)], [], [(1, 0, 0)]], 2, full=300), E.HEAT_PATH_BYTE)
    both(gpu_engine, HC.make("16", rng, 1, 1, 16, 4, [[(0, 0, 3), (15, 0, 0)]], 3, full=300), E.HEAT_PATH_VECTOR)


def test_every_refusal_launches_nothing(gpu_engine):
    eng = gpu_engine
    c = NAMED["vector: r = 1"]
    n, oh, ow = c.canvases.shape[:3]
    both(eng, c, E.HEAT_PATH_VECTOR)
    # (buffers that hold the largest sizes asked for below: the binding's own "canvas holds" / "state holds" come before the library's words)
    canvas = eng.alloc(n * oh * 4097 * 3)
    canvas.upload(np.full(canvas.nbytes, 0x5A, np.uint8))
    state = eng.alloc(4 * oh * 4097 * 4)
    state.upload(np.full(state.nbytes, 0x5A, np.uint8))
    ok = dict(n=n, oh=oh, ow=ow, planes=1, points=c.points, first=c.first, valid=c.valid, **c.call)
    crowd = np.tile(np.array([[3, 3, 0]], np.int32), (65, 1))
    cases = [(dict(n=0, first=[0], valid=[]), "at least one frame"), (dict(oh=0), "oh = 0 outside"), (dict(ow=4097), "ow = 4097 outside"),
             (dict(planes=0), "planes = 0 outside"), (dict(planes=5), "planes = 5 outside"), (dict(r=0), "r = 0 outside"), (dict(r=256), "r = 256 outside"),
             (dict(full=0), "full = 0 outside"), (dict(full=1 << 24), "full = 16777216 outside"), (dict(alpha=-1), "alpha = -1 outside"),
             (dict(alpha=257), "alpha = 257 outside"), (dict(show_mask=0), "names no plane"), (dict(show_mask=2), "at or above planes = 1"),
             (dict(first=None), "is NULL"), (dict(valid=None), "is NULL"), (dict(lut=None), "is NULL"), (dict(points=None), "the points are NULL"),
             (dict(first=[1, 2, 3, 3]), r"first\[0\] = 1"), (dict(first=[0, 2, 1, 3]), r"first\[2\] = 1 is below"),
             (dict(points=crowd, first=[0, 65, 65, 65]), "frame 0 has 65 points"), (dict(points=[[32768, 0, 0]], first=[0, 1, 1, 1]), "beyond"),
             (dict(points=[[0, -32768, 0]], first=[0, 1, 1, 1]), "beyond"), (dict(points=[[0, 0, 1]], first=[0, 1, 1, 1]), "no plane of 1"),
             (dict(valid=[1, 0, 1]), "frame 1 is not valid and carries 1 points")]
    try:
        for change, said in cases:
            a = dict(ok, **change)
            with pytest.raises(E.EngineError, match=said):
                eng.heat(canvas, a["n"], a["oh"], a["ow"], state, a["planes"], a["points"], a["first"], a["valid"],
                         r=a["r"], full=a["full"], alpha=a["alpha"], show_mask=a["show_mask"], lut=a["lut"])
        with pytest.raises(E.EngineError, match="the state overlaps the canvases"):      # maps that begin inside the canvases
            eng.heat(canvas, n, oh, ow, canvas.view(n * oh * ow * 3 - 4, oh * ow * 4), 1, c.points, c.first, c.valid, **c.call)
        with pytest.raises(E.EngineError, match="canvas holds"):
            eng.heat(canvas.view(0, 100), n, oh, ow, state, 1, c.points, c.first, c.valid, **c.call)
        with pytest.raises(E.EngineError, match="state holds"):
            eng.heat(canvas, n, oh, ow, state.view(0, 100), 1, c.points, c.first, c.valid, **c.call)
        eng.synchronize()
        assert eng.heat_last_path() == E.HEAT_PATH_VECTOR     # still the last launch's: none of these launched
        assert np.all(canvas.download(np.empty(canvas.nbytes, np.uint8)) == 0x5A)
        assert np.all(state.download(np.empty(state.nbytes, np.uint8)) == 0x5A)
    finally:
        canvas.free()
        state.free()
