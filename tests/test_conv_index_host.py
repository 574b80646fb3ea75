"""csrc/conv_index.h on the CPU: the index arithmetic all conv kernels share, through the stand-alone program
tests/conv_index_main.cpp (plain g++ and the ROCm headers for kernels.h's fill_fastdiv; no GPU, no engine library).

The program checks, and exits non-zero with one line per failed check:
* tile map — n_mtiles in {1, 7, 8, 9, 17, 64} x n_ntiles in {1, 2, 3}, over the grid 8 * ceil(n_mtiles / 8) * n_ntiles the launchers
  size: every (mt, nt) comes from exactly one valid block id, padding ids yield none and follow every valid id of their XCD
  (conv_patch_h2r.hip's persistent walk relies on it), consecutive ids of one XCD walk the channel tiles of one pixel tile first;
* origin — 8 x 16 and 16 x 16 tiles over (Ho, Wo) in {(1, 1), (8, 16), (9, 17), (20, 20)}, 2 images: the tiles cover every output
  pixel exactly once and the image index changes at image boundaries only;
* swizzle — p in 0..191: the four (tail planes: two) slot offsets are 16-byte aligned, inside the pixel's 64 (32) bytes, a permutation;
* fastdiv == n / d with fill_fastdiv's (magic, shift) for d in {1, 2, 3, 7, 18, 180, 641}, n in {0, 1, d - 1, d, d + 1, 2^31 - 1}
  and 4000 pseudo-random n.
It runs twice: as built, and built with -fsanitize=address,undefined (a plain executable; nothing is preloaded)."""
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "padel_analytics_amd" / "csrc"


@pytest.mark.parametrize("extra", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_shared_index_math(tmp_path, extra):
    exe = tmp_path / "conv_index_main"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{CSRC}", *extra,
                    str(ROOT / "tests" / "conv_index_main.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith("0 checks failed")
