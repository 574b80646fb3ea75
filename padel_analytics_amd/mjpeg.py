"""Baseline JPEG on the host: the numpy statement of the bit stream ``include/padel_hip.h`` specifies for ``pa_jpeg_encode`` and the
readable twin of csrc/jpeg_encode.hip — ``encode_host`` produces the same bytes as the kernels, and is the CPU path of
``video.MjpegSink`` (``on_device=False``), as ``render.render_host`` is for the renderer.

One frame is one baseline sequential JPEG, 4:2:0, every MCU row its own restart interval; all arithmetic is integer (the forward DCT
is the 13-bit Loeffler-Ligtenberg-Moshovitz transform libjpeg calls "islow"), so host and device agree bit for bit."""
from __future__ import annotations

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])
# ITU-T T.81 Annex K.1 / K.2, row-major
QUANT_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                       87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                       72, 92, 95, 98, 112, 100, 103, 99])
QUANT_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99]
                        + [99] * 36)
# Annex K.3 - K.6 as DHT carries them: (codes per length 1..16, symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748"
    "494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3"
    "c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")))
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], list(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a4344454647"
    "48494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9ba"
    "c2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))
HEADER_BYTES = 613
BLOCK_MAX_BYTES = 208        # 22 bits of DC + 63 x 26 bits of AC, rounded up


def huff_codes(spec):
    """(code[256], length[256]) per symbol of one table; length 0: no such symbol."""
    bits, vals = spec
    code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
    c = k = 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            code[vals[k]], length[vals[k]] = c, n
            c += 1
            k += 1
        c <<= 1
    return code, length


_CODES = {"dc": (huff_codes(DC_LUMA), huff_codes(DC_CHROMA)), "ac": (huff_codes(AC_LUMA), huff_codes(AC_CHROMA))}
_BITLEN = np.array([int(i).bit_length() for i in range(4096)], np.int64)


def quant_tables(quality: int):
    """(luma, chroma): the 64 entries of each table, row-major — libjpeg's quality rule over the Annex K tables."""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError(f"quality {quality} outside [1, 100]")
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (QUANT_LUMA, QUANT_CHROMA))


def interval_max_bytes(w: int) -> int:
    """The most bytes one restart interval of a frame of width ``w`` can take, its closing marker included (pa_jpeg_interval_bytes)."""
    return 2 * (((w + 15) // 16) * 6 * BLOCK_MAX_BYTES + 1) + 2


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct8(d, rows: bool):
    """One pass over 8 values (arrays): the row pass scales by 4, the column pass brings the total to 8."""
    odd = 11 if rows else 15
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = [None] * 8
    out[0] = (t10 + t11) * 4 if rows else _descale(t10 + t11, 2)
    out[4] = (t10 - t11) * 4 if rows else _descale(t10 - t11, 2)
    z = (t12 + t13) * 4433
    out[2] = _descale(z + t13 * 6270, odd)
    out[6] = _descale(z - t12 * 15137, odd)
    z5 = (t4 + t6 + t5 + t7) * 9633
    z1, z2 = (t4 + t7) * -7373, (t5 + t6) * -20995
    z3, z4 = (t4 + t6) * -16069 + z5, (t5 + t7) * -3196 + z5
    out[7] = _descale(t4 * 2446 + z1 + z3, odd)
    out[5] = _descale(t5 * 16819 + z2 + z4, odd)
    out[3] = _descale(t6 * 25172 + z2 + z3, odd)
    out[1] = _descale(t7 * 12299 + z1 + z4, odd)
    return out


def fdct_blocks(blocks: np.ndarray) -> np.ndarray:
    """(..., 8, 8) samples -> (..., 8, 8) coefficients scaled by 8: level shift, rows, then columns."""
    b = np.asarray(blocks).astype(np.int64) - 128
    r = np.stack(_fdct8([b[..., :, i] for i in range(8)], True), -1)
    return np.stack(_fdct8([r[..., i, :] for i in range(8)], False), -2)


def quantise_blocks(blocks: np.ndarray, q: np.ndarray) -> np.ndarray:
    """(..., 8, 8) samples -> quantised coefficients (..., 8, 8): sign(c) * ((|c| + 4 q) // (8 q))."""
    c = fdct_blocks(blocks)
    q = np.asarray(q, np.int64).reshape(8, 8)
    return np.sign(c) * ((np.abs(c) + 4 * q) // (8 * q))


def pad_plane(p: np.ndarray, unit: int) -> np.ndarray:
    """The plane completed to multiples of ``unit`` by repeating its last column and row."""
    h, w = p.shape
    return np.pad(p, ((0, -h % unit), (0, -w % unit)), mode="edge")


def planes(raw: np.ndarray, i: int, h: int, w: int, desc) -> tuple:
    """(Y, Cb, Cr) of frame ``i`` of the raw bytes ``desc`` lays out."""
    from .video import YUV_LAYOUTS, _desc_dict
    d = _desc_dict(desc)
    strided = np.lib.stride_tricks.as_strided
    cs = 2 if d["layout"] == YUV_LAYOUTS["nv12"] else 1
    f = raw[i * d["frame_stride"]:]
    return (strided(f, (h, w), (d["pitch_y"], 1)), strided(f[d["off_u"]:], (h // 2, w // 2), (d["pitch_c"], cs)),
            strided(f[d["off_v"]:], (h // 2, w // 2), (d["pitch_c"], cs)))


def _blocks(p: np.ndarray) -> np.ndarray:
    """(H, W) -> (H / 8, W / 8, 8, 8)."""
    return p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).swapaxes(1, 2)


def frame_coefficients(y, cb, cr, quality: int) -> np.ndarray:
    """(MCU rows, MCUs per row, 6, 64): the quantised coefficients of a frame in scan order (Y00 Y01 Y10 Y11 Cb Cr), zig-zag."""
    qy, qc = quant_tables(quality)
    zy = quantise_blocks(_blocks(pad_plane(np.asarray(y), 16)), qy)
    R, M = zy.shape[0] // 2, zy.shape[1] // 2
    out = np.empty((R, M, 6, 64), np.int64)
    zy = zy.reshape(R, 2, M, 2, 64)
    for k in range(4):
        out[:, :, k] = zy[:, k >> 1, :, k & 1]
    for k, p in ((4, cb), (5, cr)):
        out[:, :, k] = quantise_blocks(_blocks(pad_plane(np.asarray(p), 8)), qc).reshape(R, M, 64)
    return out[..., ZIGZAG]


def _value_bits(v, size):
    return np.where(v < 0, v - 1, v) & ((1 << size) - 1)


def interval_entries(z: np.ndarray) -> tuple:
    """(values, lengths) of the codes of one restart interval, in stream order.  ``z``: (MCUs, 6, 64) quantised coefficients,
    zig-zag.  A code and the value bits behind it are one entry."""
    m = z.shape[0]
    comp = np.array([0, 0, 0, 0, 1, 1])
    # DC: the difference to the previous block of the same component, 0 in front of the first
    diff = np.empty((m, 6), np.int64)
    yd = z[:, :4, 0].reshape(-1)
    diff[:, :4] = (yd - np.concatenate(([0], yd[:-1]))).reshape(m, 4)
    for k in (4, 5):
        diff[:, k] = z[:, k, 0] - np.concatenate(([0], z[:-1, k, 0]))
    blk = np.arange(m * 6).reshape(m, 6)
    keys, vals, lens = [], [], []
    for c in (0, 1):
        sel = comp == c
        d, b = diff[:, sel].reshape(-1), blk[:, sel].reshape(-1)
        size = _BITLEN[np.abs(d)]
        code, length = _CODES["dc"][c]
        keys.append(b * 260)
        vals.append(code[size] << size | _value_bits(d, size))
        lens.append(length[size] + size)
        # AC: the non-zero coefficients of these blocks, each with the zeros in front of it
        ac = z[:, sel, 1:].reshape(-1, 63)
        bi, pos = np.nonzero(ac)
        pos = pos + 1
        first = np.concatenate(([True], bi[1:] != bi[:-1])) if bi.size else np.zeros(0, bool)
        prev = np.where(first, 0, np.concatenate(([0], pos[:-1])))
        run = pos - prev - 1
        v = ac[bi, pos - 1]
        size = _BITLEN[np.abs(v)]
        code, length = _CODES["ac"][c]
        for zrl in range(3):                                     # up to three ZRL (16 zeros each) in front of the symbol
            keys.append(b[bi] * 260 + pos * 4 + zrl)
            vals.append(np.full(bi.size, code[0xf0]))
            lens.append(np.where((run >> 4) > zrl, length[0xf0], 0))
        sym = (run & 15) << 4 | size
        keys.append(b[bi] * 260 + pos * 4 + 3)
        vals.append(code[sym] << size | _value_bits(v, size))
        lens.append(length[sym] + size)
        # EOB unless the block's last coefficient is non-zero
        eob = ac[:, 62] == 0
        keys.append(b[eob] * 260 + 256)
        vals.append(np.full(int(eob.sum()), code[0]))
        lens.append(np.full(int(eob.sum()), length[0]))
    keys, vals, lens = np.concatenate(keys), np.concatenate(vals), np.concatenate(lens)
    order = np.argsort(keys, kind="stable")
    return vals[order], lens[order]


def pack_interval(vals: np.ndarray, lens: np.ndarray) -> bytes:
    """The codes MSB first, the last byte padded with 1-bits, every 0xFF followed by 0x00."""
    total = int(lens.sum())
    start = np.cumsum(lens) - lens
    j = np.arange(total) - np.repeat(start, lens)
    bits = (np.repeat(vals, lens) >> (np.repeat(lens, lens) - 1 - j)) & 1
    bits = np.concatenate((bits, np.ones(-total % 8, np.int64))).astype(np.uint8)
    return np.packbits(bits).tobytes().replace(b"\xff", b"\xff\x00")


def frame_header(h: int, w: int, quality: int) -> bytes:
    """SOI .. SOS: 613 bytes."""
    qy, qc = quant_tables(quality)
    be16 = lambda v: int(v).to_bytes(2, "big")
    out = b"\xff\xd8" + b"\xff\xe0" + be16(16) + b"JFIF\0" + bytes([1, 1, 0]) + be16(1) + be16(1) + bytes([0, 0])
    out += b"\xff\xdb" + be16(2 + 2 * 65) + bytes([0]) + bytes(qy[ZIGZAG].tolist()) + bytes([1]) + bytes(qc[ZIGZAG].tolist())
    out += b"\xff\xc0" + be16(17) + bytes([8]) + be16(h) + be16(w) + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    dht = b"".join(bytes([ident]) + bytes(spec[0]) + bytes(spec[1])
                   for ident, spec in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)))
    out += b"\xff\xc4" + be16(2 + len(dht)) + dht
    out += b"\xff\xdd" + be16(4) + be16((w + 15) // 16)
    out += b"\xff\xda" + be16(12) + bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert len(out) == HEADER_BYTES
    return out


def frame_intervals(y, cb, cr, quality: int) -> list:
    """The stuffed bytes of every restart interval of one frame, without markers."""
    return [pack_interval(*interval_entries(row)) for row in frame_coefficients(y, cb, cr, quality)]


def encode_frame(y, cb, cr, quality: int = 90) -> bytes:
    h, w = np.asarray(y).shape
    ivls = frame_intervals(y, cb, cr, quality)
    out = [frame_header(h, w, quality)]
    for r, data in enumerate(ivls):
        out += [data, b"\xff\xd9" if r == len(ivls) - 1 else bytes([0xff, 0xd0 + (r & 7)])]
    return b"".join(out)


def check(n: int, h: int, w: int, desc, quality: int) -> None:
    """ValueError for what ``pa_jpeg_encode`` refuses (the geometry refusals are ``video.yuv_span``'s)."""
    from .video import yuv_span
    if w > 2560:
        raise ValueError(f"width {w} is beyond the 2560 pixels the encoder supports")
    if not 1 <= int(quality) <= 100:
        raise ValueError(f"quality {quality} outside [1, 100]")
    yuv_span(n, h, w, desc)


def encode_host(raw, n: int, h: int, w: int, desc, quality: int = 90) -> tuple:
    """``n`` frames of 8-bit YUV 4:2:0 in the 1-D byte array ``raw``, laid out by ``desc`` (``video.yuv_desc``; the decode
    coefficients are not used) -> (the JPEGs back to back as a uint8 array, offsets (n + 1,) int64) — what ``Engine.jpeg_encode``
    returns, byte for byte."""
    from .video import yuv_span
    raw = np.asarray(raw)
    if raw.dtype != np.uint8 or raw.ndim != 1:
        raise ValueError("raw YUV bytes must be a 1-D uint8 array")
    check(n, h, w, desc, quality)
    if yuv_span(n, h, w, desc) > raw.size:
        raise ValueError(f"{n} frames as described span {yuv_span(n, h, w, desc)} bytes, the array holds {raw.size}")
    frames = [encode_frame(*planes(raw, i, h, w, desc), quality) for i in range(n)]
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum([len(f) for f in frames])
    return np.frombuffer(b"".join(frames), np.uint8), offsets
