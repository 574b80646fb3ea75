"""Pillow as a yardstick for the Motion-JPEG writer, on the CPU (no GPU, no engine): for every case of tests/mjpeg_cases.py the mean
squared error of Pillow-decode(ours) and of Pillow-decode(Pillow's own encoding of the same planes, same quality, 4:2:0, standard
tables) against the source planes, and the two byte counts.  Writes profiles/mjpeg_parity.txt; the byte margins of
tests/test_mjpeg_host.py (BYTE_MARGIN) are taken from its last table.

    python tools/mjpeg_parity.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import mjpeg_cases as MC                     # noqa: E402
from tests.test_mjpeg_host import parity                # noqa: E402


def main() -> None:
    lines = ["Motion-JPEG writer against Pillow (libjpeg), measured on the CPU with mjpeg.encode_host — the bytes the kernels produce",
             "(tests/test_gpu_mjpeg.py).  Per case, summed over its 3 frames: MSE of Pillow-decode(ours) and of Pillow-decode(Pillow's own",
             "encoding: same planes, chroma repeated 2 x 2, same quality, subsampling=2, optimize=False) against the source planes; bytes of",
             "ours and of Pillow's.", "",
             f"{'size':>9} {'layout':>6} {'content':>11} {'mse ours':>10} {'mse pillow':>10} {'bytes ours':>10} {'bytes pil':>10} {'excess':>8}  pixels"]
    worst, identical = {}, True
    for w, h in MC.SIZES:
        for layout in MC.LAYOUTS:
            for content in MC.CONTENTS:
                se = np.zeros(2)
                nbytes = np.zeros(2, np.int64)
                same = True
                count = 0
                for ours, theirs, src, b_ours, b_ref in parity(content, w, h, layout):
                    se += [((ours.astype(np.float64) - src) ** 2).sum(), ((theirs.astype(np.float64) - src) ** 2).sum()]
                    count += src.size
                    nbytes += [b_ours, b_ref]
                    same &= bool(np.array_equal(ours, theirs))
                identical &= same
                excess = nbytes[0] / nbytes[1] - 1
                worst[(w, h)] = max(worst.get((w, h), -1.0), excess)
                lines.append(f"{w:>4}x{h:<4} {layout:>6} {content:>11} {se[0] / count:>10.3f} {se[1] / count:>10.3f} {nbytes[0]:>10} {nbytes[1]:>10} "
                             f"{100 * excess:>7.2f}%  {'identical' if same else 'DIFFERENT'}")
    lines += ["", "Decoded pixels: " + ("IDENTICAL to Pillow's in every case — the test asserts identity, so the MSE margin is 0."
                                        if identical else "NOT identical in every case."),
              "Bytes: ours carry DRI, one RSTm per interval and each interval's padding; where the size is no multiple of 16 they also code",
              "the blocks that lie wholly outside the frame from repeated edge pixels, which libjpeg codes as empty blocks (34x18, 2x2).",
              "Margin per size = max(1 %, 2 x the largest excess over layouts and contents):", ""]
    for (w, h), e in worst.items():
        lines.append(f"{w:>4}x{h:<4} largest excess {100 * e:>6.2f}%   margin {100 * max(0.01, 2 * e):>6.2f}%")
    out = ROOT / "profiles" / "mjpeg_parity.txt"
    out.write_text("\n".join(lines) + "\n")
    print("\n".join(lines[-8:]))
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
