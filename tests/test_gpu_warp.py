"""``Engine.warp`` (csrc/warp.hip, ``pa_warp_perspective``) on the GPU against its numpy twin ``topdown.warp_host``, bit for bit, the
store path asserted per case through ``Engine.warp_last_path``: identity, half a pixel and a horizon inside the canvas on the byte
path and on the 16-byte path, one-pixel sources, a source wholly outside, frames with their own matrices and one that is not valid,
a misaligned destination between sentinel bytes, ``ow = 16 k + 1``, a canvas larger than one pass of the launch's grid-stride loop,
the size limits, and every refusal — which launches nothing.  Equality with the twin is what shows that the device rounds every
product and sum on its own (the file is built with -ffp-contract=off): a fused multiply-add moves coordinates across 1 / 32 cells."""
import numpy as np
import pytest

from padel_analytics_amd import engine as E, topdown as T
from tests import warp_cases as W

pytestmark = pytest.mark.gpu

PAD = 64            # sentinel bytes kept in front of and behind the destination
FILL = (7, 99, 201)


def gpu_warp(eng, frames, matrices, valid, oh, ow, fill=FILL, dst_shift=0):
    """-> (canvases, path): the frames uploaded, warped into a buffer filled with 0x5A ``PAD + dst_shift`` bytes in; the bytes on
    both sides of the destination must come back untouched, and the source unchanged."""
    n, h, w = frames.shape[:3]
    src = eng.alloc(frames.nbytes)
    src.upload(frames)
    span = n * oh * ow * 3
    dst = eng.alloc(span + 2 * PAD + dst_shift)
    dst.upload(np.full(dst.nbytes, 0x5A, np.uint8))
    try:
        eng.warp(src, n, h, w, matrices, valid, dst.view(PAD + dst_shift, span), oh, ow, fill=fill)
        path = eng.warp_last_path()
        whole = dst.download(np.empty(dst.nbytes, np.uint8))
        assert np.all(whole[:PAD + dst_shift] == 0x5A) and np.all(whole[PAD + dst_shift + span:] == 0x5A), "bytes around dst were written"
        assert np.array_equal(src.download(np.empty(frames.nbytes, np.uint8)), frames.reshape(-1)), "the source was written"
    finally:
        eng.synchronize()
        src.free()
        dst.free()
    return whole[PAD + dst_shift:PAD + dst_shift + span].reshape(n, oh, ow, 3), path


def both(eng, frames, matrices, valid, oh, ow, want_path, fill=FILL, dst_shift=0):
    matrices = np.asarray(matrices, np.float64).reshape(-1, 3, 3)
    want = T.warp_host(frames, matrices, valid, oh, ow, fill)
    got, path = gpu_warp(eng, frames, matrices, valid, oh, ow, fill, dst_shift)
    assert path == want_path
    assert np.array_equal(got, want), f"{int((got != want).any(axis=-1).sum())} of {got.shape[0] * oh * ow} pixels differ"
    return got


@pytest.fixture(scope="module")
def source():
    return W.frames_of(1, 37, 53, 21)                        # 37 rows of 53 pixels


MATRICES = {
    "identity": lambda oh, ow: np.eye(3),
    "half a pixel": lambda oh, ow: W.translation(0.5, 0.5),
    "horizon inside": lambda oh, ow: W.horizon_matrix(37, 53, oh, ow),
}


@pytest.mark.parametrize("name", list(MATRICES))
@pytest.mark.parametrize("oh, ow, path", [(29, 41, E.WARP_PATH_BYTE), (32, 48, E.WARP_PATH_VECTOR)])
def test_against_the_twin_on_both_store_paths(gpu_engine, source, name, oh, ow, path):
    got = both(gpu_engine, source, MATRICES[name](oh, ow), [1], oh, ow, path)
    filled = (got == np.array(FILL, np.uint8)).all(axis=-1)
    if name == "identity":
        assert np.array_equal(got[0, :oh, :ow], source[0, :oh, :ow]) and not filled.any()
    if name == "horizon inside":                             # above the horizon fill, below it the picture
        assert filled[0, :int(0.4 * oh)].all() and not filled[0, -1].all()


def test_one_pixel_sources(gpu_engine):
    one = np.array([[[[200, 100, 50]]]], np.uint8)
    got = both(gpu_engine, one, np.eye(3), [1], 1, 1, E.WARP_PATH_BYTE)
    assert got.tolist() == [[[[200, 100, 50]]]]
    # 7 x 5 around it: canvas (u, v) reads (u / 2 - 1.25, v / 2 - 0.75).  Columns 1..4 and rows 0..3 fall into the cells -1 and 0, where
    # the pixel weighs 8 / 32 or 24 / 32 each way: three mixtures with fill (64, 192 and 576 of 1024), and fill everywhere else
    m = np.array([[0.5, 0, -1.25], [0, 0.5, -0.75], [0, 0, 1.0]])
    got = both(gpu_engine, one, m, [1], 5, 7, E.WARP_PATH_BYTE)
    mix = lambda k: tuple((np.array(FILL) * (1024 - k) + np.array([200, 100, 50]) * k + 512) >> 10)
    assert {tuple(int(c) for c in p) for p in got.reshape(-1, 3)} == {FILL, mix(64), mix(192), mix(576)}
    assert tuple(got[0, 4, 6]) == FILL and tuple(got[0, 1, 2]) == mix(576) and tuple(got[0, 0, 1]) == mix(64)


def test_a_source_wholly_outside(gpu_engine, source):
    for m in (W.translation(500, 0), W.translation(0, -38), W.translation(-54, 0)):
        for (oh, ow, path) in ((9, 11, E.WARP_PATH_BYTE), (4, 16, E.WARP_PATH_VECTOR)):
            got = both(gpu_engine, source, m, [1], oh, ow, path)
            assert (got == np.array(FILL, np.uint8)).all()


@pytest.mark.parametrize("oh, ow, path", [(13, 19, E.WARP_PATH_BYTE), (12, 32, E.WARP_PATH_VECTOR)])
def test_three_frames_with_their_own_matrices_the_middle_one_not_valid(gpu_engine, oh, ow, path):
    frames = W.frames_of(3, 23, 31, 5)
    m = np.stack([W.translation(2.25, -1.5), np.full((3, 3), np.nan), W.horizon_matrix(23, 31, oh, ow, at=0.2)])
    got = both(gpu_engine, frames, m, [1, 0, 1], oh, ow, path)
    assert (got[1] == np.array(FILL, np.uint8)).all() and not np.array_equal(got[0], got[2])


def test_a_misaligned_destination_takes_the_byte_path(gpu_engine, source):
    for shift in (1, 4, 15):                                  # 48 columns would allow 16-byte stores: the address does not
        both(gpu_engine, source, W.horizon_matrix(37, 53, 32, 48), [1], 32, 48, E.WARP_PATH_BYTE, dst_shift=shift)
    both(gpu_engine, source, W.horizon_matrix(37, 53, 32, 48), [1], 32, 48, E.WARP_PATH_VECTOR, dst_shift=16)


def test_a_width_of_16_k_plus_1(gpu_engine, source):
    both(gpu_engine, source, W.translation(-3.4, 2.2), [1], 7, 65, E.WARP_PATH_BYTE)
    both(gpu_engine, source, W.translation(-3.4, 2.2), [1], 7, 17, E.WARP_PATH_BYTE)


@pytest.mark.parametrize("oh, ow, path", [(760, 700, E.WARP_PATH_BYTE), (2060, 4096, E.WARP_PATH_VECTOR)])
def test_a_canvas_larger_than_one_pass_of_the_grid(gpu_engine, source, oh, ow, path):
    """A launch covers 2048 x 256 threads per frame at once: 524 288 pixels on the byte path, 16 times as many on the 16-byte path.
    760 x 700 = 532 000 and 2060 x 4096 / 16 = 527 360 threads take a second pass of the loop."""
    assert oh * ow // (16 if path == E.WARP_PATH_VECTOR else 1) > 2048 * 256
    m = np.array([[53 / ow, 0.002, -0.3], [0.001, 37 / oh, -0.2], [0, 0.1 / oh, 1.0]])
    both(gpu_engine, source, m, [1], oh, ow, path)


def test_the_size_limits(gpu_engine):
    frames = W.frames_of(1, 2, 4096, 9)                       # 4096 wide, 2 high -> 2 wide, 4096 high
    m = np.array([[0.0, 1.0, 0.3], [1.0, 0.0, -0.2], [0, 0, 1.0]])      # the transpose, a little off the grid
    got = both(gpu_engine, frames, m, [1], 4096, 2, E.WARP_PATH_BYTE)
    assert not (got == np.array(FILL, np.uint8)).all(axis=-1)[0, :4095, 1].any()


def test_every_refusal_launches_nothing(gpu_engine, source):
    eng = gpu_engine
    # (buffers that hold the largest sizes asked for below: the binding's own "src holds" / "dst holds" come before the library's words)
    src = eng.alloc(37 * 4097 * 3)
    src.upload(source)
    dst = eng.alloc(29 * 4097 * 3)
    dst.upload(np.full(dst.nbytes, 0x5A, np.uint8))
    both(eng, source, np.eye(3), [1], 32, 48, E.WARP_PATH_VECTOR)
    nan = np.eye(3)
    nan[2, 1] = np.nan
    ok = dict(n=1, h=37, w=53, matrices=np.eye(3), valid=[1], oh=29, ow=41)
    cases = [(dict(n=0, matrices=np.zeros((0, 9)), valid=[]), "at least one frame"), (dict(h=0), "h = 0 outside"), (dict(w=4097), "w = 4097 outside"),
             (dict(oh=0), "oh = 0 outside"), (dict(ow=4097), "ow = 4097 outside"), (dict(matrices=None), "is NULL"), (dict(valid=None), "is NULL"),
             (dict(matrices=nan), "entry 7 of frame 0's matrix is not finite")]
    try:
        for change, said in cases:
            a = dict(ok, **change)
            with pytest.raises(E.EngineError, match=said):
                eng.warp(src, a["n"], a["h"], a["w"], a["matrices"], a["valid"], dst, a["oh"], a["ow"])
        with pytest.raises(E.EngineError, match="dst overlaps src"):      # a canvas that begins inside the frames
            eng.warp(src, 1, 37, 53, np.eye(3), [1], src.view(37 * 53 * 3 - 1, 65), 1, 21)
        with pytest.raises(E.EngineError, match="src holds"):
            eng.warp(src.view(0, 100), 1, 37, 53, np.eye(3), [1], dst, 29, 41)
        with pytest.raises(E.EngineError, match="dst holds"):
            eng.warp(src, 1, 37, 53, np.eye(3), [1], dst.view(0, 29 * 41 * 3), 30, 41)
        eng.synchronize()
        assert eng.warp_last_path() == E.WARP_PATH_VECTOR     # still the last launch's: none of these launched
        assert np.all(dst.download(np.empty(dst.nbytes, np.uint8)) == 0x5A)
        assert np.array_equal(src.download(np.empty(source.nbytes, np.uint8)), source.reshape(-1))
    finally:
        src.free()
        dst.free()
