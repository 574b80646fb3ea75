"""Which kernel a forced tile id runs, written down by hand from the kernels' documented support conditions (the comments
of csrc/kernels.h and of the dispatchers, the shapes every kernel file says it takes) — NOT by calling the engine.  The GPU
sweeps compare it with what the engine reports per launch (``Model.profile_rows()``: ``tile`` / ``family``), in both
directions: a silent fall-through this table does not know fails, and so does a tile running where it is documented not to.
The CPU test tests/test_tile_coverage.py computes from this table alone whether the parametrised sweeps reach every tile
NATIVELY (launched id == requested id) on every class of shape its kernel supports.

Pure Python; imports neither the engine nor numpy.

A case is the sweeps' tuple (B, H, W, cin, cout, k, stride, act, residual); unit graphs put a stride-2 conv's output on the
next level (Ho = H // 2).  ``path``: "h2" | "bx3" | "tap" | "f16".  ``w_single``: the h2 conv runs its two-product form
(PA_CONV_W_SINGLE weights and tuning w_single = 1)."""

ACT_NONE, ACT_SILU, ACT_RELU, ACT_SIGMOID, ACT_LEAKY = 0, 1, 2, 3, 4
ACTS = (ACT_NONE, ACT_SILU, ACT_RELU, ACT_SIGMOID, ACT_LEAKY)

# ---- workgroup tiles: ("lin", pixels, channels) = BM consecutive output pixels; ("patch", rows, cols, channels) = a patch of the map
_FP32_IDS = {6: (64, 128), 7: (64, 96), 9: (128, 64), 10: (128, 64), 11: (128, 32), 12: (128, 16), 13: (128, 96), 14: (128, 128),
             15: (128, 64), 20: (128, 48), 25: (64, 80)}
SHAPES = {
    "tap": {v: ("lin",) + _FP32_IDS[v] for v in (6, 7, 9, 10, 11, 12, 13, 14, 15, 20)},
    # bf16x3: the fp32 ids (3-stage ring), + 200 the 2-stage ring, 30x the 8 x 16 patch kernel with 3 / 4 / 6 fragments
    "bx3": {**{v: ("lin",) + _FP32_IDS[v] for v in (6, 7, 9, 11, 12, 13, 14, 20, 25)},
            **{200 + v: ("lin",) + _FP32_IDS[v] for v in (6, 7, 9, 11, 20, 25)}, 213: ("lin", 128, 96),
            303: ("patch", 8, 16, 48), 304: ("patch", 8, 16, 64), 306: ("patch", 8, 16, 96)},
    "h2": {207: ("lin", 64, 96), 209: ("lin", 128, 64), 211: ("lin", 128, 32), 213: ("lin", 128, 96), 220: ("lin", 128, 48), 225: ("lin", 64, 80),
           239: ("lin", 128, 64), 243: ("lin", 128, 96),                                     # deep activation ring, 1x1
           244: ("lin", 128, 96), 245: ("lin", 128, 192), 247: ("lin", 64, 192),              # register weights, 1x1
           246: ("lin", 128, 192), 248: ("lin", 64, 192),                                     # register weights, stride-2 3x3
           303: ("patch", 8, 16, 48), 304: ("patch", 8, 16, 64), 313: ("patch", 8, 16, 48),   # patch kernel (31x: pipelined schedule)
           323: ("patch", 8, 16, 96), 324: ("patch", 8, 16, 96), 325: ("patch", 8, 16, 64),   # quad kernel / its register-weights forms
           341: ("patch", 16, 16, 16), 342: ("patch", 16, 16, 32), 343: ("patch", 16, 16, 48)},   # wide patch kernel, cin 16 / 32 / 48
    # fp16: + 30 the larger per-wave tiles, + 40 the same tiles with 64-channel k-steps; 30x patch (8 x 16), 32x quad (16 x 16)
    "f16": {6: ("lin", 64, 128), 7: ("lin", 64, 96), 9: ("lin", 128, 64), 11: ("lin", 128, 32), 12: ("lin", 128, 16), 20: ("lin", 128, 48),
            30: ("lin", 128, 128), 31: ("lin", 128, 96), 32: ("lin", 128, 64),
            46: ("lin", 64, 128), 47: ("lin", 64, 96), 49: ("lin", 128, 64), 51: ("lin", 128, 32), 60: ("lin", 128, 48),
            70: ("lin", 128, 128), 71: ("lin", 128, 96), 72: ("lin", 128, 64),
            303: ("patch", 8, 16, 48), 304: ("patch", 8, 16, 64), 306: ("patch", 8, 16, 96),
            323: ("patch", 16, 16, 48), 324: ("patch", 16, 16, 64), 326: ("patch", 16, 16, 96)},
}

# channel fragments (16 channels) per WAVE of every fp16 tile, from the launcher tables of csrc/conv_tap16.hip (launch_conv_t16) and
# csrc/conv_patch16.hip (launch_conv_p16): f16_epilogue stores fragment pairs with 16 bytes and an odd last fragment with 8
F16_NF = {6: 4, 7: 3, 9: 4, 11: 2, 12: 1, 20: 3, 30: 4, 31: 3, 32: 2,
          46: 4, 47: 3, 49: 4, 51: 2, 60: 3, 70: 4, 71: 3, 72: 2,
          303: 3, 304: 4, 306: 6, 323: 3, 324: 4, 326: 6}
assert set(F16_NF) == set(SHAPES["f16"])

PATCH_FAMILIES = ("h2p", "h2q", "h2r", "h2v", "h2w", "bx3p", "p16", "p16q")
NO_K_LOOP = ("h2v", "h2w")          # the wide patch kernels hold the whole K extent (cin <= 48) in LDS: no K loop to exercise


def _h2(tile, k, s, cin, w_single):
    s1_3x3 = k == 3 and s == 1                   # every unit graph keeps a stride-1 conv at its input's size, no absorbed upsample
    whole = cin % 32 == 0
    if 341 <= tile <= 343:                        # wide patch kernel: stride-1 3x3 with 16 / 32 / 48 input channels
        if s1_3x3 and cin in (16, 32, 48):       # register-weights form h2v; its 3-fragment tile exists for two-product layers only
            return ("h2w" if tile == 343 and not w_single else "h2v"), tile
        tile = 303
    if tile == 324:                               # 96-channel register-weights quad tiles: two-product layers, whole chunks, >= 2
        if s1_3x3 and whole and cin >= 64 and w_single:
            return "h2r", 324
        tile = 323
    if tile == 325:                               # 64-channel ones: two or three products
        if s1_3x3 and whole and cin >= 64:
            return "h2r", 325
        tile = 304
    if tile == 323:                               # quad patch kernel: stride-1 3x3, cin % 32 == 0
        if s1_3x3 and whole and cin >= 32:
            return "h2q", 323
        tile = 303
    if 300 <= tile < 400:                         # patch kernel: every stride-1 3x3; elsewhere its tap sibling
        if s1_3x3:
            return "h2p", tile
        tile = {303: 220, 313: 220, 304: 209}.get(tile, 213)
    if tile in (246, 248):                        # register-weights ring machine, stride-2 3x3: two products, whole chunks
        if k == 3 and s == 2 and whole and cin >= 32 and w_single:
            return "h2s3", tile
        tile = 213
    if tile in (244, 245, 247):                   # ... 1x1: two products, whole chunks, at least two
        if k == 1 and s == 1 and whole and cin >= 64 and w_single:
            return "h2s", tile
        tile = 243
    if tile in (243, 239):                        # deep activation ring: 1x1 only; other kernel sizes: the plain tile
        if k == 1:
            return "h2d", tile
        tile -= 30
    assert tile in (207, 209, 211, 213, 220, 225), tile
    return "h2t", tile


def expected(path, tile, case, w_single=False):
    """(family, tile) of the kernel a forced ``tile`` launches on ``case``."""
    B, H, W, cin, cout, k, s, act, res = case
    assert tile in SHAPES[path], (path, tile)
    if path == "tap":
        return "tap", tile
    if path == "bx3":
        if 300 <= tile < 400:                     # patch kernel: stride-1 3x3 (any cin % 16 == 0); elsewhere a 2-stage tap tile
            if k == 3 and s == 1:
                return "bx3p", tile
            tile = {303: 220, 304: 209, 306: 206}[tile]
        return "bx3t", tile
    if path == "f16":
        if 300 <= tile < 400:                     # fp16 patch kernels: stride-1 3x3, cin % 32 == 0 (every fp16 slice)
            if k == 3 and s == 1:
                return ("p16q" if tile >= 320 else "p16"), tile
            tile = {303: 20, 304: 9}.get(tile, 31)
        return ("tap16d" if tile >= 40 else "tap16"), tile
    assert path == "h2", path
    return _h2(tile, k, s, cin, bool(w_single))


def out_hw(case):
    B, H, W, cin, cout, k, s, act, res = case
    return (H // 2, W // 2) if s == 2 else (H, W)


def ksteps(path, case):
    """64-byte k-steps of the K walk: 32 channels x one tap; a 3x3's 16-channel tail pairs its 9 taps into 5 steps."""
    cin, k = case[3], case[5]
    if path == "f16":
        return (cin + 31) // 32 * k * k
    return (cin // 32) * 9 + (5 if cin & 16 else 0) if k == 3 else (cin + 31) // 32


def classes(path, family, tile, case):
    """Shape classes a NATIVE run of ``tile`` on ``case`` exercises.

    full              whole pixel tiles and whole channel tiles only
    m_tail            (linear pixel tiles) the last pixel tile is partial
    patch_y, patch_x  (patch tiles) partial patches at the bottom / right edge
    n_tail            cout is not a multiple of the tile's channels;  n_tail16: cout % 16 != 0 (a partial fragment)
    res / nores       with / without the fused residual
    long_k            the K loop wraps: >= 2 accumulation blocks of 9 k-steps (ring kernels), >= 9 32-channel chunks (patch kernels)
    """
    B, H, W, cin, cout, k, s, act, res = case
    shape = SHAPES[path][tile]
    Ho, Wo = out_hw(case)
    cls = {"res" if res else "nores"}
    if shape[0] == "lin":
        bn = shape[2]
        part_m = (B * Ho * Wo) % shape[1] != 0
        if part_m:
            cls.add("m_tail")
    else:
        bn = shape[3]
        py, px = Ho % shape[1] != 0, Wo % shape[2] != 0
        part_m = py or px
        if py:
            cls.add("patch_y")
        if px:
            cls.add("patch_x")
    if cout % bn:
        cls.add("n_tail")
    if cout % 16:
        cls.add("n_tail16")
    if not part_m and cout % bn == 0:
        cls.add("full")
    if family not in NO_K_LOOP:
        if (cin // 32 >= 9) if family in PATCH_FAMILIES else (ksteps(path, case) >= 10):
            cls.add("long_k")
    return cls


def required_classes(path, family, tile):
    req = {"full", "n_tail", "n_tail16", "res", "nores"}
    req |= {"m_tail"} if SHAPES[path][tile][0] == "lin" else {"patch_y", "patch_x"}
    if family not in NO_K_LOOP:
        req.add("long_k")
    return req


def h2_store_paths(family, tile, case):
    """Store paths of csrc/h2_common.h a native h2 run takes when it writes PAIRS (a non-head buffer) at 16-aligned slices:
    a workgroup whose fragments lie inside the tensor and the channel matrix takes the 16-byte path (with or without the
    residual load), every other one the element-wise path."""
    cls = classes("h2", family, tile, case)
    if "full" in cls:
        return {"fast_res" if case[8] else "fast"}
    return {"slow"}          # (its interior workgroups still take the fast path)


F16_STORE_PATHS = ("pair16", "tail8", "pair16_res", "tail8_res", "f32", "slow", "slow_f32")


def f16_store_paths(family, tile, case, head):
    """Store paths of csrc/f16_epilogue.h a native fp16 run takes at 8-aligned slices.  ``head``: "f16" (the conv writes halves) or
    "f32" (it writes the fp32 head buffer itself).  The kernels' ``fast`` predicates (conv_tap16.hip: PADEL_T16_FINISH,
    conv_patch16.hip) hold for a workgroup whose pixels and channel fragments all exist, i.e. for every workgroup of a ``full``
    case; ``f16_epilogue`` then takes

      pair16 / pair16_res   one 16-byte store per fragment pair (NF >= 2), with a residual also one 16-byte load
      tail8 / tail8_res     the 8-byte store (and residual load) of fragment NF - 1 of an odd NF
      f32                   16-byte fp32 stores — an fp32 head without residual (``wide`` is false for out_f32 with a residual)

    and everything else the element-wise path, ``slow`` or ``slow_f32`` (its interior workgroups still take the fast paths: the
    rule of ``h2_store_paths``)."""
    assert head in ("f16", "f32"), head
    cls = classes("f16", family, tile, case)
    res = bool(case[8])
    if head == "f32":
        return {"f32"} if "full" in cls and not res else {"slow_f32"}
    if "full" not in cls:
        return {"slow"}
    nf, sfx = F16_NF[tile], "_res" if res else ""
    return ({"pair16" + sfx} if nf >= 2 else set()) | ({"tail8" + sfx} if nf & 1 else set())


def f16_paths_of_tile(tile):
    """Every path of ``f16_store_paths`` the tile's NF allows (both heads, with and without residual)."""
    nf = F16_NF[tile]
    fast = ({"pair16", "pair16_res"} if nf >= 2 else set()) | ({"tail8", "tail8_res"} if nf & 1 else set())
    return fast | {"f32", "slow", "slow_f32"}


def native(path, tile, case, w_single=False):
    return expected(path, tile, case, w_single)[1] == tile


def plan(path, tiles, case, w_single=False):
    """The forced runs of a sweep on one case: ``[(tile, (family, launched))]`` without the DUPLICATES — a tile that resolves to
    (family, tile') is dropped where the same sweep runs tile' under its own id on this case (the same kernel on the same
    operands a second time).  Nothing else is ever dropped."""
    runs = []
    for t in tiles:
        fam, got = expected(path, t, case, w_single)
        if got != t and got in tiles and expected(path, got, case, w_single) == (fam, got):
            continue
        runs.append((t, (fam, got)))
    return runs


def coverage_gaps(path, tiles, runs):
    """``runs``: iterable of (case, w_single).  Returns the list of unfilled cells: (tile, family, class) for every tile id, over
    the families it runs natively in this sweep's modes, and (family, "act", a) for every family without activation ``a``."""
    seen, acts, fams = {}, {}, {}
    for case, ws in runs:
        for t in tiles:
            fam, got = expected(path, t, case, ws)
            if got != t:
                continue
            seen.setdefault((t, fam), set()).update(classes(path, fam, t, case))
            acts.setdefault(fam, set()).add(case[7])
            fams.setdefault(t, set()).add(fam)
    gaps = []
    for t in tiles:
        if t not in fams:
            gaps.append((t, None, "never runs natively"))
            continue
        for fam in sorted(fams[t]):
            for c in sorted(required_classes(path, fam, t) - seen[(t, fam)]):
                gaps.append((t, fam, c))
    for fam in sorted(acts):
        for a in ACTS:
            if a not in acts[fam]:
                gaps.append((fam, "act", a))
    return gaps
