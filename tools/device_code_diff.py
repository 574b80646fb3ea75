#!/usr/bin/env python3
"""Is the device code of two source trees the same?

    python tools/device_code_diff.py <tree_a> <tree_b> [--work DIR] [--only conv_tap.hip ...] [--reuse-a] [--reuse-b]

Every .hip translation unit of csrc/build.sh's ALL list is compiled to gfx950 assembly (device side only) in both trees, once
plain and, where the file or a header of csrc/ names them, once more with -DPADEL_H2P_PROBES -DPADEL_BX3_PROBES.  Comment lines
and trailing `;` comments are dropped (they carry paths and the compiler's own remarks), the hash in the name of the
__hip_cuid_<hash> marker object (a digest of the source text, no code) is blanked, and the two texts are compared line by line:
kernel symbols, instructions, kernel descriptors, LDS and register counts all live in what remains.  One line per translation
unit: "identical", or the first differing lines.  Exit status 1 on any difference.  The assembly is only compared, never searched.
A refactor of the kernels' source runs this against a checkout of its parent commit.

--work DIR keeps the assembly (DIR/a, DIR/b); --reuse-a takes DIR/a/*.s from an earlier run instead of compiling tree_a again,
--reuse-b the same for tree_b (both: compare only)."""
import argparse
import difflib
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

CSRC = Path("padel_analytics_amd") / "csrc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S"]
PROBES = ["-DPADEL_H2P_PROBES", "-DPADEL_BX3_PROBES"]
JOBS = 16
SHOWN = 12          # differing lines printed per translation unit
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")       # the compilation unit's id symbol: a hash of the source text


def translation_units(tree):
    m = re.search(r'^ALL="([^"]*)"', (tree / CSRC / "build.sh").read_text(), re.M)
    return m.group(1).split()


def has_probes(tree, tu):
    texts = [(tree / CSRC / tu).read_text()] + [h.read_text() for h in sorted((tree / CSRC).glob("*.h"))]
    return any(p[2:] in t for p in PROBES for t in texts)


def compile_asm(tree, tu, extra, out):
    r = subprocess.run(["hipcc", *FLAGS, *extra, tu, "-o", str(out.resolve())], cwd=tree / CSRC, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{tree / CSRC / tu}: hipcc failed\n{r.stderr[-2000:]}")


def code_lines(path):
    out = []
    for ln in CUID.sub("__hip_cuid_", path.read_text()).split("\n"):
        ln = ln.split(";", 1)[0].rstrip()
        if ln and not ln.lstrip().startswith("//"):
            out.append(ln)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tree_a", type=Path)
    ap.add_argument("tree_b", type=Path)
    ap.add_argument("--work", type=Path, help="keep the assembly here")
    ap.add_argument("--only", nargs="+", metavar="TU", help="these translation units instead of build.sh's whole list")
    ap.add_argument("--reuse-a", action="store_true", help="use the assembly of tree_a that an earlier run left in --work")
    ap.add_argument("--reuse-b", action="store_true", help="the same for tree_b")
    args = ap.parse_args()
    tmp = None if args.work else tempfile.TemporaryDirectory()
    work = args.work or Path(tmp.name)
    tus = args.only or translation_units(args.tree_b)
    if not args.only and translation_units(args.tree_a) != tus:
        print("the two build.sh list different translation units", file=sys.stderr)
        return 1
    units = [(tu, tag, extra) for tu in tus for tag, extra in (("", []), (" +probes", PROBES))
             if not extra or has_probes(args.tree_a, tu) or has_probes(args.tree_b, tu)]
    jobs = []
    for side, tree in (("a", args.tree_a), ("b", args.tree_b)):
        (work / side).mkdir(parents=True, exist_ok=True)
        for tu, tag, extra in units:
            out = work / side / (Path(tu).stem + (".probes" if extra else "") + ".s")
            if not (out.exists() and (args.reuse_a if side == "a" else args.reuse_b)):
                jobs.append((tree, tu, extra, out))
    with ThreadPoolExecutor(JOBS) as pool:
        for f in [pool.submit(compile_asm, *j) for j in jobs]:
            f.result()
    different = symbols = probe_symbols = 0
    for tu, tag, extra in units:
        name = Path(tu).stem + (".probes" if extra else "") + ".s"
        a, b = code_lines(work / "a" / name), code_lines(work / "b" / name)
        kernels = sum(1 for ln in b if ln.lstrip().startswith(".amdhsa_kernel "))
        if extra:
            probe_symbols += kernels
        else:
            symbols += kernels
        if a == b:
            print(f"{tu}{tag}: identical ({len(b)} lines, {kernels} kernels)")
            continue
        different += 1
        delta = [d for d in difflib.unified_diff(a, b, "a", "b", n=0, lineterm="") if not d.startswith(("---", "+++"))] \
            if len(a) + len(b) < 400000 else next(([f"line {i + 1}:", "-" + x, "+" + y] for i, (x, y) in enumerate(zip(a, b)) if x != y),
                                                   [f"one text is a prefix of the other ({len(a)} / {len(b)} lines)"])
        print(f"{tu}{tag}: DIFFERENT ({len(a)} / {len(b)} lines); first differing lines:")
        for d in delta[:SHOWN]:
            print("    " + d)
    print(f"{len(units)} builds of {len(tus)} translation units, {symbols} kernel symbols (probe builds: {probe_symbols}): " +
          ("all identical" if not different else f"{different} DIFFERENT"))
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main())
