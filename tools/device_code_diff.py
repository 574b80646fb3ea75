#!/usr/bin/env python3
"""Is the device code of two source trees the same?

    python tools/device_code_diff.py <tree_a> <tree_b> [--work DIR] [--only conv_tap.hip ...] [--reuse-a] [--reuse-b]
                                     [--per-kernel [--dropped KERNEL:I=V,... ...]]

Every .hip translation unit of csrc/build.sh's ALL list is compiled to gfx950 assembly (device side only) in both trees.  Comment
lines and trailing `;` comments are dropped (they carry paths and the compiler's own remarks), the hash in the name of the
__hip_cuid_<hash> marker object (a digest of the source text, no code) is blanked, and the two texts are compared line by line:
kernel symbols, instructions, kernel descriptors, LDS and register counts all live in what remains.  One line per translation
unit: "identical", or the first differing lines.  Exit status 1 on any difference.  The assembly is only compared, never searched.
A refactor of the kernels' source runs this against a checkout of its parent commit (tree_a).

--per-kernel: for a change that REMOVES instantiations or template parameters — the whole text of such a translation unit cannot
match.  Where it does not, the text is cut into functions (from a function's label to the end of its resource symbols: the
instructions, the .amdhsa_kernel descriptor with the register counts, LDS and scratch sizes); a function of tree_b is paired with
the function of tree_a of the same demangled name (c++filt), its own symbol is replaced by a placeholder and the function's
ordinal in local labels (.LBB<n>_<m>, .Lfunc_end<n>: it shifts when earlier functions vanish) is blanked, labels counted through
the whole unit (.Lpost_getpc<n>, .Ltmp<n>) are renumbered from the function's first; then line by line as above.  --dropped conv_h2s_kernel:1=0,2=2 says that tree_b dropped template arguments 1 and 2 (counted from 0) of that kernel
and that tree_a's instantiations with the values 0 and 2 there are the ones that live on under the shorter name.  Passes when
every function of tree_b has a counterpart with the same lines; the functions of tree_a without one are listed by name.

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
JOBS = 16
SHOWN = 12          # differing lines printed per translation unit
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")       # the compilation unit's id symbol: a hash of the source text


def translation_units(tree):
    m = re.search(r'^ALL="([^"]*)"', (tree / CSRC / "build.sh").read_text(), re.M)
    return m.group(1).split()


def compile_asm(tree, tu, out):
    r = subprocess.run(["hipcc", *FLAGS, tu, "-o", str(out.resolve())], cwd=tree / CSRC, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{tree / CSRC / tu}: hipcc failed\n{r.stderr[-2000:]}")


def code_lines(path):
    out = []
    for ln in CUID.sub("__hip_cuid_", path.read_text()).split("\n"):
        ln = ln.split(";", 1)[0].rstrip()
        if ln and not ln.lstrip().startswith("//"):
            out.append(ln)
    return out


FUNC_TYPE = re.compile(r"\s*\.type\s+(\S+),@function$")
ORDINAL = re.compile(r"\.(LBB|Lfunc_begin|Lfunc_end)\d+")
COUNTED = re.compile(r"\.(Lpost_getpc|Ltmp)(\d+)")      # numbered through the whole translation unit: renumbered from the function's first


def functions(lines):
    """{symbol: its lines, from the label to the last of its resource symbols}, the symbol and the function's ordinal blanked"""
    out = {}
    i = 0
    while i < len(lines):
        m = FUNC_TYPE.match(lines[i])
        i += 1
        if not m:
            continue
        sym = m.group(1)
        end = next((j for j in range(i, len(lines)) if ".AMDGPU.csdata" in lines[j] or FUNC_TYPE.match(lines[j])), len(lines))
        seen = {}
        out[sym] = [COUNTED.sub(lambda c: f".{c.group(1)}#{seen.setdefault(c.group(0), len(seen))}",
                                ORDINAL.sub(r".\1", ln.replace(sym, "<function>"))) for ln in lines[i:end]]
        i = end
    return out


def demangled(symbols):
    r = subprocess.run(["c++filt"], input="\n".join(symbols), capture_output=True, text=True, check=True)
    return dict(zip(symbols, r.stdout.split("\n")))


def drop_arguments(name, dropped):
    """the name tree_b gives an instantiation of tree_a, None: tree_b has dropped it (--dropped)"""
    m = re.match(r"(.*?\b(\w+))<([^<>]*)>(.*)$", name)
    if not m or m.group(2) not in dropped:
        return name
    args = m.group(3).split(", ")
    spec = dropped[m.group(2)]
    if any(i >= len(args) or args[i] != v for i, v in spec.items()):
        return None
    return f"{m.group(1)}<{', '.join(a for i, a in enumerate(args) if i not in spec)}>{m.group(4)}"


def diff_functions(a, b, dropped):
    """-> (functions of b, [(name, first differing lines)], [names of b without a counterpart], [names of a without one])"""
    fa, fb = functions(a), functions(b)
    names_a = demangled(list(fa))
    by_name = {}
    for sym, name in names_a.items():
        by_name.setdefault(drop_arguments(name, dropped), []).append(sym)
    differ, missing, used = [], [], set()
    for sym, name in demangled(list(fb)).items():
        twins = by_name.get(name, [])
        if len(twins) != 1:
            missing.append(name + (f" ({len(twins)} candidates)" if twins else ""))
            continue
        used.add(twins[0])
        if fa[twins[0]] != fb[sym]:
            differ.append((name, [d for d in difflib.unified_diff(fa[twins[0]], fb[sym], "a", "b", n=0, lineterm="")
                                  if not d.startswith(("---", "+++"))][:SHOWN]))
    return len(fb), differ, missing, sorted(names_a[s] for s in fa if s not in used)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tree_a", type=Path)
    ap.add_argument("tree_b", type=Path)
    ap.add_argument("--work", type=Path, help="keep the assembly here")
    ap.add_argument("--only", nargs="+", metavar="TU", help="these translation units instead of build.sh's whole list")
    ap.add_argument("--reuse-a", action="store_true", help="use the assembly of tree_a that an earlier run left in --work")
    ap.add_argument("--reuse-b", action="store_true", help="the same for tree_b")
    ap.add_argument("--per-kernel", action="store_true", help="where the whole texts differ, compare function by function")
    ap.add_argument("--dropped", nargs="+", default=[], metavar="KERNEL:I=V,...",
                    help="template arguments tree_b dropped from a kernel, and the values they had in the instantiations that live on")
    args = ap.parse_args()
    tmp = None if args.work else tempfile.TemporaryDirectory()
    work = args.work or Path(tmp.name)
    tus = args.only or translation_units(args.tree_b)
    if not args.only and translation_units(args.tree_a) != tus:
        print("the two build.sh list different translation units", file=sys.stderr)
        return 1
    dropped = {k: {int(i): v for i, v in (iv.split("=") for iv in spec.split(","))} for k, spec in (d.split(":") for d in args.dropped)}
    jobs = []
    for side, tree in (("a", args.tree_a), ("b", args.tree_b)):
        (work / side).mkdir(parents=True, exist_ok=True)
        for tu in tus:
            out = work / side / (Path(tu).stem + ".s")
            if not (out.exists() and (args.reuse_a if side == "a" else args.reuse_b)):
                jobs.append((tree, tu, out))
    with ThreadPoolExecutor(JOBS) as pool:
        for f in [pool.submit(compile_asm, *j) for j in jobs]:
            f.result()
    different = symbols = 0
    for tu in tus:
        name = Path(tu).stem + ".s"
        a, b = code_lines(work / "a" / name), code_lines(work / "b" / name)
        kernels = sum(1 for ln in b if ln.lstrip().startswith(".amdhsa_kernel "))
        symbols += kernels
        if a == b:
            print(f"{tu}: identical ({len(b)} lines, {kernels} kernels)")
            continue
        if args.per_kernel:
            n, differ, missing, gone = diff_functions(a, b, dropped)
            ok = not differ and not missing
            print(f"{tu}: " + (f"all {n} functions identical to tree_a's" if ok else
                               f"{len(differ)} of {n} functions DIFFERENT, {len(missing)} without a counterpart in tree_a") +
                  f"; {len(gone)} functions of tree_a without a counterpart" + (":" if gone else ""))
            for g in gone:
                print("    gone: " + g)
            for m in missing:
                print("    NO COUNTERPART: " + m)
            for fn, delta in differ:
                print(f"    DIFFERENT: {fn}")
                for d in delta:
                    print("        " + d)
            different += 0 if ok else 1
            continue
        different += 1
        delta = [d for d in difflib.unified_diff(a, b, "a", "b", n=0, lineterm="") if not d.startswith(("---", "+++"))] \
            if len(a) + len(b) < 400000 else next(([f"line {i + 1}:", "-" + x, "+" + y] for i, (x, y) in enumerate(zip(a, b)) if x != y),
                                                   [f"one text is a prefix of the other ({len(a)} / {len(b)} lines)"])
        print(f"{tu}: DIFFERENT ({len(a)} / {len(b)} lines); first differing lines:")
        for d in delta[:SHOWN]:
            print("    " + d)
    print(f"{len(tus)} translation units, {symbols} kernel symbols: " +
          ("all identical" if not different else f"{different} DIFFERENT"))
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main())
