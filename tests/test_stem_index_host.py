"""The input-patch index math of the fused stem + layer-1 kernel (csrc/conv_index.h: ``stem_patch_*``, ``stem_lq_*``,
``stem_pair_*``) on the CPU, through the stand-alone program tests/stem_index_main.cpp (plain g++; no GPU, no engine library).

The program stages a random u8 NHWC4 frame — the middle one of three, so that a row taken from a neighbouring frame shows — into
a host copy of the kernel's LDS patch with those functions, chunk by chunk as the kernel's threads do, then builds every MFMA
operand slot the way a lane does (its four words, one byte permute per slot pair, ``0x6400 | byte`` minus 1024) and compares it
with the direct per-slot formula of the weight-ring instantiations: slot k = 3 tap + colour of stem position p is that byte of
input pixel (4 oy0 - 3 + 2 srow + dy, 4 ox0 - 3 + 2 scol + dx), 0 outside the image and for k >= 27.  Images 32 x 32 and 64 x 160,
every tile (all four corners, every edge, the interior, the partial last column), every p < 297, every k < 32; also: a chunk is
wholly inside or wholly outside the image, every word lies inside the patch, nothing is written past it.
It runs twice: as built, and built with -fsanitize=address,undefined (a plain executable; nothing is preloaded)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "padel_analytics_amd" / "csrc"


@pytest.mark.parametrize("extra", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_stem_patch_index_math(tmp_path, extra):
    exe = tmp_path / "stem_index_main"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{CSRC}", *extra,
                    str(ROOT / "tests" / "stem_index_main.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith(" 0 checks failed")
