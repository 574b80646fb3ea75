"""CPU twins of two claims the fused SPPF kernels and the fp16 helper kernels rest on (csrc/kernels_misc.hip, csrc/graph_plan.cpp).

1. ``sppf_h2_kernel`` / ``sppf_f16_kernel`` compute the row of pixel p without an integer division:
   ``y = (int)(((float)p + 0.5f) * (1.0f / (float)W))``.  The same float32 operations in numpy, for every map width and every pixel
   the kernels can be launched with (two LDS planes of 16 bytes per pixel inside ``kSppfMaxLds``, read from the source), against
   ``p // W``.  tests/test_gpu_helpers.py samples a dozen widths on the device; this covers all of them.
2. fp16 graphs: the engine refuses a pool / upsample on a buffer whose width is not a multiple of 8 halves.  No graph the builders
   produce has such a buffer."""
import re
from pathlib import Path

import numpy as np

from padel_analytics_amd import graph as G, yolo_arch

SRC = Path(__file__).resolve().parents[1] / "padel_analytics_amd" / "csrc" / "kernels_misc.hip"


def max_pixels():
    m = re.search(r"constexpr\s+size_t\s+kSppfMaxLds\s*=\s*(\d+)\s*\*\s*(\d+)\s*;", SRC.read_text())
    assert m, "kSppfMaxLds not found in kernels_misc.hip"
    lds = int(m.group(1)) * int(m.group(2))
    return lds // 32                      # sppf_f16_kernel: 2 planes x 16 bytes per pixel (sppf_h2_kernel: 2 x 32, half as many pixels)


def test_row_index_without_division_is_exact_for_every_launchable_map():
    n = max_pixels()
    assert n >= 4800
    half, one = np.float32(0.5), np.float32(1.0)
    for W in range(1, n + 1):
        p = np.arange((n // W) * W, dtype=np.int64)
        inv_w = one / np.float32(W)
        y = ((p.astype(np.float32) + half) * inv_w).astype(np.int32)
        assert y.dtype == np.int32 and (p.astype(np.float32) + half).dtype == np.float32
        bad = np.flatnonzero(y != p // W)
        assert bad.size == 0, f"W = {W}: pixel {int(p[bad[0]])} gets row {int(y[bad[0]])}, not {int(p[bad[0]] // W)}"


def _fp16_graphs():
    for scale in ("n", "s", "m", "l", "x"):
        for nc, kpt in ((80, None), (1, (13, 3))):
            yield f"yolov8{scale}-{'pose' if kpt else 'detect'}", G.build_yolov8(yolo_arch.synth_state_dict(scale, nc, kpt, seed=0), nc, kpt, dtype="f16")


def test_fp16_graphs_keep_helper_buffers_a_multiple_of_8_wide():
    """What validate_desc (csrc/graph_plan.cpp) refuses for fp16 graphs, checked on every graph the builders make.  (Only build_yolov8
    has an fp16 form: build_tracknet and build_inpaintnet make fp32 / h2 graphs.)"""
    seen = 0
    for name, g in _fp16_graphs():
        assert g.dtype == G.DTYPE_F16
        for i, o in enumerate(g.ops):
            if o["kind"] in (G.OP_SPPF_POOL, G.OP_UPSAMPLE2X, G.OP_MAXPOOL2):
                seen += 1
                for b in (o["in_buf"], o["out_buf"]):
                    assert g.bufs[b][1] % 8 == 0, f"{name}: op {i} (kind {o['kind']}) uses buffer {b} of {g.bufs[b][1]} channels"
    assert seen > 0
