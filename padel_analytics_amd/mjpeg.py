"""Baseline JPEG on the host: the numpy statement of the bit stream ``include/padel_hip.h`` specifies for ``pa_jpeg_encode`` and the
readable twin of csrc/jpeg_encode.hip — ``encode_host`` produces the same bytes as the kernels, and is the CPU path of
``video.MjpegSink`` (``on_device=False``), as ``render.render_host`` is for the renderer.

One frame is one baseline sequential JPEG, 4:2:0, every MCU row its own restart interval; all arithmetic is integer (the forward DCT
is the 13-bit Loeffler-Ligtenberg-Moshovitz transform libjpeg calls "islow"), so host and device agree bit for bit.

The second half of the module reads: ``parse_frame`` / ``decode_host`` are the twins of csrc/jpeg_parse.cpp and csrc/jpeg_decode.hip
(``pa_jpeg_decode``: any baseline 4:2:0 JPEG, not only the writer's), ``index_file`` finds the frames of an ``.avi`` / ``.mjpeg`` file."""
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


# ---------------------------------------------------------------------------------------------- reading
# The numpy statement of what ``include/padel_hip.h`` specifies for ``pa_jpeg_decode``: ``parse_frame`` is the twin of
# csrc/jpeg_parse.cpp, ``decode_host`` of csrc/jpeg_entropy.h + csrc/jpeg_decode.hip (the same bytes) and the CPU path of
# ``video.MjpegClip`` (``on_device=False``); ``index_file`` reads the containers ``video.MjpegSink`` writes.
ST_CODE, ST_INDEX, ST_SIZE, ST_DATA, ST_MARKERS = 1, 2, 4, 8, 16          # PA_JPEG_ST_*: bits of a frame's status word
DEC_MAX_DIM = 4096                                                       # PA_JPEG_DEC_MAX_DIM
DEC_MAX_BYTES = 1 << 27                                                  # PA_JPEG_DEC_MAX_BYTES


class NotMjpeg(ValueError):
    """The container holds no Motion-JPEG stream (``video`` then tries ``cv2``)."""


def _check_huff(bits, nvals_have: int, name: str) -> int:
    code = total = 0
    for n in range(1, 17):
        total += bits[n - 1]
        code += bits[n - 1]
        if code > 1 << n:
            raise ValueError(f"jpeg: DHT table {name} has more codes of length {n} than fit")
        code <<= 1
    if total > 256:
        raise ValueError(f"jpeg: DHT table {name} lists {total} symbols")
    if total > nvals_have:
        raise ValueError(f"jpeg: truncated header: DHT ends inside the symbols of table {name}")
    return total


def parse_frame(jpeg) -> dict:
    """The markers of one baseline JPEG -> its description: ``w``, ``h``, ``mcus_x``, ``mcus_y``, ``restart_interval``, ``status`` (0 or
    ``ST_MARKERS``), ``default_huffman``, ``scan_begin`` / ``scan_end``, ``quant`` (3, 64) per component in zig-zag order, ``comp_dc`` /
    ``comp_ac``, ``dc`` / ``ac`` (two ``(bits, vals)`` each) and ``intervals``: (begin, end, first MCU, MCUs) of every restart interval.
    ValueError with its reason for what ``pa_jpeg_parse`` refuses."""
    p = bytes(jpeg)
    size = len(p)
    if size < 4 or p[:2] != b"\xff\xd8":
        raise ValueError(f"jpeg: no SOI marker at the start ({size} bytes)")
    if size > DEC_MAX_BYTES:
        raise ValueError(f"jpeg: a frame of {size} bytes is beyond the {DEC_MAX_BYTES} the decoder counts bits for")
    qt, dc, ac = {}, {}, {}
    sof = None
    ri = 0
    pos = 2
    while True:
        if pos + 2 > size:
            raise ValueError(f"jpeg: truncated header: the bytes end at {size}, before any scan")
        if p[pos] != 0xff:
            raise ValueError(f"jpeg: truncated header: byte {pos} is 0x{p[pos]:02x} where a marker belongs")
        m = p[pos + 1]
        if m == 0xff:
            pos += 1
            continue
        if m == 0x01 or 0xd0 <= m <= 0xd8:
            pos += 2
            continue
        if m == 0xd9:
            raise ValueError(f"jpeg: EOI at byte {pos}, before any scan")
        if pos + 4 > size:
            raise ValueError(f"jpeg: truncated header: the bytes end inside the segment of marker FF{m:02X}")
        L = p[pos + 2] << 8 | p[pos + 3]
        if L < 2 or pos + 2 + L > size:
            raise ValueError(f"jpeg: truncated header: the segment of marker FF{m:02X} at byte {pos} claims {L} bytes, {size - pos - 2} remain")
        s = p[pos + 4:pos + 2 + L]
        n = L - 2
        if m in (0xc2, 0xc6):
            raise ValueError(f"jpeg: progressive frame (SOF{m - 0xc0}): baseline sequential only")
        if m in (0xc1, 0xc5):
            raise ValueError(f"jpeg: extended sequential frame (SOF{m - 0xc0}): baseline sequential only")
        if m in (0xc3, 0xc7):
            raise ValueError(f"jpeg: lossless frame (SOF{m - 0xc0}): baseline sequential only")
        if m == 0xcc or 0xc9 <= m <= 0xcf:
            raise ValueError(f"jpeg: arithmetic coding (marker FF{m:02X}): Huffman coding only")
        if m == 0xc0:
            if sof is not None:
                raise ValueError(f"jpeg: a second SOF0 at byte {pos}: one frame per JPEG")
            if n < 6:
                raise ValueError(f"jpeg: truncated header: SOF0 of {n} bytes")
            if s[0] != 8:
                raise ValueError(f"jpeg: {s[0]}-bit samples: 8-bit data only")
            h, w, nf = s[1] << 8 | s[2], s[3] << 8 | s[4], s[5]
            if nf != 3:
                raise ValueError(f"jpeg: {nf} component(s): three (Y, Cb, Cr) are needed")
            if n < 15:
                raise ValueError(f"jpeg: truncated header: SOF0 of {n} bytes for 3 components")
            if not (1 <= w <= DEC_MAX_DIM and 1 <= h <= DEC_MAX_DIM):
                raise ValueError(f"jpeg: {w} x {h} frame outside 1 .. {DEC_MAX_DIM} pixels a side")
            comps = []
            for c in range(3):
                cid, hv, tq = s[6 + 3 * c], s[7 + 3 * c], s[8 + 3 * c]
                if hv != (0x22 if c == 0 else 0x11):
                    raise ValueError(f"jpeg: sampling {hv >> 4}x{hv & 15} of component {c}: 4:2:0 only (Y 2x2, Cb and Cr 1x1)")
                if tq > 3:
                    raise ValueError(f"jpeg: component {c} names quantisation table {tq}")
                comps.append((cid, tq))
            sof = (w, h, comps)
        elif m == 0xdb:
            i = 0
            while i < n:
                pq, tq = s[i] >> 4, s[i] & 15
                if pq:
                    raise ValueError(f"jpeg: 16-bit quantisation table {tq}: 8-bit DQT only")
                if tq > 3:
                    raise ValueError(f"jpeg: DQT defines table {tq}")
                if i + 65 > n:
                    raise ValueError(f"jpeg: truncated header: DQT ends inside table {tq}")
                qt[tq] = np.frombuffer(s[i + 1:i + 65], np.uint8)
                i += 65
        elif m == 0xc4:
            i = 0
            while i < n:
                tc, th = s[i] >> 4, s[i] & 15
                if tc > 1 or th > 1:
                    raise ValueError(f"jpeg: DHT defines table class {tc} id {th}: baseline has DC / AC tables 0 and 1")
                if i + 17 > n:
                    raise ValueError(f"jpeg: truncated header: DHT ends inside table {tc}/{th}")
                bits = list(s[i + 1:i + 17])
                total = _check_huff(bits, n - i - 17, f"{tc}/{th}")
                (ac if tc else dc)[th] = (bits, list(s[i + 17:i + 17 + total]))
                i += 17 + total
        elif m == 0xdd:
            if n != 2:
                raise ValueError(f"jpeg: truncated header: DRI of {n} bytes")
            ri = s[0] << 8 | s[1]
        elif m == 0xda:
            if sof is None:
                raise ValueError(f"jpeg: SOS at byte {pos} before any SOF0")
            if n < 1:
                raise ValueError("jpeg: truncated header: empty SOS")
            if s[0] != 3:
                raise ValueError(f"jpeg: a scan of {s[0]} component(s): more than one scan is not supported (one interleaved scan of all three)")
            if n != 10:
                raise ValueError(f"jpeg: truncated header: SOS of {n} bytes for 3 components")
            comp_dc, comp_ac = [], []
            for c in range(3):
                if s[1 + 2 * c] != sof[2][c][0]:
                    raise ValueError(f"jpeg: the scan lists component id {s[1 + 2 * c]} where the frame has {sof[2][c][0]}")
                td, ta = s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15
                if td > 1 or ta > 1:
                    raise ValueError(f"jpeg: component {c} names Huffman tables {td} / {ta}: baseline has 0 and 1")
                comp_dc.append(td)
                comp_ac.append(ta)
            if s[7] != 0 or s[8] != 63 or s[9] != 0:
                raise ValueError(f"jpeg: scan with Ss {s[7]}, Se {s[8]}, Ah/Al 0x{s[9]:02x}: one sequential scan (0, 63, 0) only")
            pos += 2 + L
            break
        pos += 2 + L
    w, h, comps = sof
    for c in range(3):
        if comps[c][1] not in qt:
            raise ValueError(f"jpeg: missing table: component {c} names quantisation table {comps[c][1]}, which no DQT defined")
    default = not dc and not ac
    if default:
        dc, ac = {0: DC_LUMA, 1: DC_CHROMA}, {0: AC_LUMA, 1: AC_CHROMA}
    for c in range(3):
        if comp_dc[c] not in dc:
            raise ValueError(f"jpeg: missing table: component {c} names DC Huffman table {comp_dc[c]}, which no DHT defined")
        if comp_ac[c] not in ac:
            raise ValueError(f"jpeg: missing table: component {c} names AC Huffman table {comp_ac[c]}, which no DHT defined")
    # the entropy-coded data: split at RSTm, ended by any other marker (or by the end of the bytes)
    segs = []
    i = seg = pos
    while True:
        i = p.find(b"\xff", i)
        if i < 0 or i + 1 >= size:
            i = size
            break
        m = p[i + 1]
        if m == 0:
            i += 2
        elif m == 0xff:
            i += 1
        elif 0xd0 <= m <= 0xd7:
            segs.append((seg, i))
            i += 2
            seg = i
        else:
            break
    segs.append((seg, i))
    j = i
    while j + 4 <= size and p[j] == 0xff:
        m = p[j + 1]
        if m == 0xd9:
            break
        if m == 0xda:
            raise ValueError(f"jpeg: a second SOS at byte {j}: more than one scan is not supported")
        j += 1 if m == 0xff else 2 + (p[j + 2] << 8 | p[j + 3])
    mcus_x, mcus_y = (w + 15) // 16, (h + 15) // 16
    total = mcus_x * mcus_y
    step = ri or total
    expect = (total + step - 1) // step
    intervals = [(segs[k] if k < len(segs) else (i, i)) + (k * step, min(step, total - k * step)) for k in range(expect)]
    empty = ([0] * 16, [])
    return dict(w=w, h=h, mcus_x=mcus_x, mcus_y=mcus_y, restart_interval=ri, n_intervals=expect, default_huffman=int(default),
                status=0 if len(segs) == expect else ST_MARKERS, scan_begin=pos, scan_end=i,
                quant=np.stack([qt[comps[c][1]] for c in range(3)]), comp_dc=comp_dc, comp_ac=comp_ac,
                dc=[dc.get(t, empty) for t in (0, 1)], ac=[ac.get(t, empty) for t in (0, 1)], intervals=intervals)


_LUTS: dict = {}


def _huff_lut(spec) -> tuple:
    """(length[65536], symbol[65536]) by the 16 bits ahead; length 0: no code of the table matches."""
    bits, vals = spec
    key = (bytes(bits), bytes(vals))
    hit = _LUTS.get(key)
    if hit is None:
        length, sym = np.zeros(65536, np.int64), np.zeros(65536, np.int64)
        code = k = 0
        for n in range(1, 17):
            for _ in range(bits[n - 1]):
                length[code << (16 - n):(code + 1) << (16 - n)] = n
                sym[code << (16 - n):(code + 1) << (16 - n)] = vals[k] if k < len(vals) else 0
                code += 1
                k += 1
            code <<= 1
        if len(_LUTS) > 64:
            _LUTS.clear()
        hit = _LUTS[key] = (length.tolist(), sym.tolist())
    return hit


def decode_interval(data: bytes, mcus: int, dc_luts, ac_luts) -> tuple:
    """The stuffed bytes of one restart interval -> ((mcus, 6, 64) int16 coefficients in zig-zag order, status).  ``dc_luts`` /
    ``ac_luts``: ``_huff_lut`` of each of the three components.  From the block that cannot be decoded on, zeros."""
    import re
    m = re.search(rb"\xff(?!\x00)", data)              # FF 00 is the byte FF, any other FF ends the data
    if m:
        data = data[:m.start()]
    data = data.replace(b"\xff\x00", b"\xff")
    fed = 8 * len(data)
    b = np.frombuffer(data + b"\0\0\0", np.uint8).astype(np.int64)
    w24 = b[:-2] << 16 | b[1:-1] << 8 | b[2:]
    at = np.arange(fed)
    ahead = ((w24[at >> 3] >> (8 - (at & 7))) & 0xffff).tolist()          # the 16 bits ahead of every position; 0 past the end
    coef = np.zeros((mcus * 6, 64), np.int16)
    pred = [0, 0, 0]
    pos = 0
    for blk in range(mcus * 6):
        c = 0 if blk % 6 < 4 else blk % 6 - 3
        (dlen, dsym), (alen, asym) = dc_luts[c], ac_luts[c]
        v = ahead[pos] if pos < fed else 0
        if not dlen[v]:
            return coef.reshape(mcus, 6, 64), ST_CODE
        pos += dlen[v]
        s = dsym[v]
        if s > 11:
            return coef.reshape(mcus, 6, 64), ST_SIZE
        p = pred[c]
        if s:
            bits = (ahead[pos] if pos < fed else 0) >> (16 - s)
            pos += s
            p += bits if bits >= 1 << (s - 1) else bits - (1 << s) + 1
        out = [0] * 64
        out[0] = ((p + 32768) & 0xffff) - 32768
        k = 1
        st = 0
        while k < 64:
            v = ahead[pos] if pos < fed else 0
            if not alen[v]:
                st = ST_CODE
                break
            pos += alen[v]
            rs = asym[v]
            s = rs & 15
            if s == 0:
                if rs != 0xf0:
                    break
                k += 16
                continue
            if s > 10:
                st = ST_SIZE
                break
            k += rs >> 4
            if k > 63:
                st = ST_INDEX
                break
            bits = (ahead[pos] if pos < fed else 0) >> (16 - s)
            pos += s
            out[k] = bits if bits >= 1 << (s - 1) else bits - (1 << s) + 1
            k += 1
        if not st and k > 64:
            st = ST_INDEX
        if not st and pos > fed:
            st = ST_DATA
        if st:
            return coef.reshape(mcus, 6, 64), st
        pred[c] = p
        coef[blk] = out
    return coef.reshape(mcus, 6, 64), 0


def frame_coefficients_of(jpeg, info=None) -> tuple:
    """((MCUs, 6, 64) int16 coefficients of a frame in scan order, zig-zag; its status word)."""
    p = bytes(jpeg)
    info = info or parse_frame(p)
    dc_luts = [_huff_lut(info["dc"][t]) for t in info["comp_dc"]]
    ac_luts = [_huff_lut(info["ac"][t]) for t in info["comp_ac"]]
    coef = np.zeros((info["mcus_x"] * info["mcus_y"], 6, 64), np.int16)
    status = info["status"]
    for begin, end, first, mcus in info["intervals"]:
        coef[first:first + mcus], st = decode_interval(p[begin:end], mcus, dc_luts, ac_luts)
        status |= st
    return coef, status


def _idct8(d, s: int):
    """One pass over 8 int32 arrays with descale shift ``s`` (int32 arithmetic, wrapping)."""
    d0, d1, d2, d3, d4, d5, d6, d7 = d
    z1 = (d2 + d6) * 4433
    t2, t3 = z1 - d6 * 15137, z1 + d2 * 6270
    t0, t1 = (d0 + d4) << 13, (d0 - d4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = d7, d5, d3, d1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + (z1 + z3), a1 + (z2 + z4), a2 + (z2 + z3), a3 + (z1 + z4)
    half = np.int32(1 << (s - 1))
    return [(x + half) >> s for x in (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3)]


def idct_blocks(coef: np.ndarray, q: np.ndarray) -> np.ndarray:
    """(..., 64) coefficients in zig-zag order, ``q`` (64,) in zig-zag order -> (..., 8, 8) int32, the IDCT output before + 128."""
    with np.errstate(over="ignore"):
        z = coef.astype(np.int32) * q.astype(np.int32)
        b = np.zeros(z.shape, np.int32)
        b[..., ZIGZAG] = z
        b = b.reshape(z.shape[:-1] + (8, 8))
        cols = np.stack(_idct8([b[..., i, :] for i in range(8)], 11), -2)
        return np.stack(_idct8([cols[..., :, i] for i in range(8)], 18), -1)


def _upsample(c: np.ndarray, h: int, w: int) -> np.ndarray:
    """"h2v2 fancy": the chroma plane of its real size -> (h, w) int32."""
    c = c.astype(np.int32)
    ch, cw = c.shape
    up, down = c[np.maximum(np.arange(ch) - 1, 0)], c[np.minimum(np.arange(ch) + 1, ch - 1)]
    s = np.empty((2 * ch, cw), np.int32)
    s[0::2], s[1::2] = 3 * c + up, 3 * c + down
    left, right = s[:, np.maximum(np.arange(cw) - 1, 0)], s[:, np.minimum(np.arange(cw) + 1, cw - 1)]
    out = np.empty((2 * ch, 2 * cw), np.int32)
    out[:, 0::2], out[:, 1::2] = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4
    return out[:h, :w]


def decode_frame(jpeg, stats: dict = None) -> tuple:
    """One JPEG -> ((h, w, 3) uint8 BGR, status).  ``stats``: receives ``max_abs_idct``, the largest |IDCT output| of the frame."""
    info = parse_frame(jpeg)
    coef, status = frame_coefficients_of(jpeg, info)
    w, h, mx, my = info["w"], info["h"], info["mcus_x"], info["mcus_y"]
    coef = coef.reshape(my, mx, 6, 64)
    peak = 0
    planes = []
    for c, ks in enumerate(((0, 1, 2, 3), (4,), (5,))):
        x = idct_blocks(coef[:, :, ks, :], info["quant"][c])                      # (my, mx, len(ks), 8, 8)
        peak = max(peak, int(np.abs(x.astype(np.int64)).max()))
        with np.errstate(over="ignore"):
            x = np.clip(x + np.int32(128), 0, 255)
        if c == 0:
            x = x.reshape(my, mx, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(my * 16, mx * 16)
        else:
            x = x.reshape(my, mx, 8, 8).transpose(0, 2, 1, 3).reshape(my * 8, mx * 8)
        planes.append(x)
    if stats is not None:
        stats["max_abs_idct"] = max(stats.get("max_abs_idct", 0), peak)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    y = planes[0][:h, :w]
    cb, cr = _upsample(planes[1][:ch, :cw], h, w) - 128, _upsample(planes[2][:ch, :cw], h, w) - 128
    out = np.empty((h, w, 3), np.uint8)
    out[..., 0] = np.clip(y + ((116130 * cb + 32768) >> 16), 0, 255)
    out[..., 1] = np.clip(y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255)
    out[..., 2] = np.clip(y + ((91881 * cr + 32768) >> 16), 0, 255)
    return out, status


def decode_host_status(data, offsets, stats: dict = None) -> tuple:
    """The JPEGs ``data[offsets[i]:offsets[i + 1]]`` -> ((n, h, w, 3) uint8 BGR, status (n,) int32) — what ``Engine.jpeg_decode``
    writes and returns, byte for byte.  ValueError for what ``pa_jpeg_decode`` refuses."""
    data = np.asarray(data, np.uint8) if not isinstance(data, (bytes, bytearray)) else np.frombuffer(data, np.uint8)
    n = len(offsets) - 1
    if n < 1:
        raise ValueError(f"n = {n} frames")
    frames, status = [], np.zeros(n, np.int32)
    for i in range(n):
        try:
            f, status[i] = decode_frame(data[int(offsets[i]):int(offsets[i + 1])].tobytes(), stats)
        except ValueError as e:
            raise ValueError(f"frame {i}: {e}") from None
        if frames and f.shape != frames[0].shape:
            raise ValueError(f"frame {i} is {f.shape[1]} x {f.shape[0]}, frame 0 {frames[0].shape[1]} x {frames[0].shape[0]}: frame sizes differ "
                             f"within the clip")
        frames.append(f)
    return np.stack(frames), status


def decode_host(data, offsets) -> np.ndarray:
    """(n, h, w, 3) uint8 BGR of the JPEGs ``data[offsets[i]:offsets[i + 1]]``: the numpy twin of ``Engine.jpeg_decode``."""
    return decode_host_status(data, offsets)[0]


# ---- containers
class MjpegIndex:
    """Where the frames of a Motion-JPEG file (and the parts it continues in) are: ``entries[i]`` = (file, offset, size); ``w`` / ``h``
    from the first frame's SOF0, ``fps`` from the container."""

    def __init__(self, paths, entries, fps: int, buffers=None):
        self.paths, self.entries, self.fps = list(paths), list(entries), int(fps)
        self._maps = list(buffers) if buffers is not None else [None] * len(self.paths)
        if not self.entries:
            raise ValueError(f"{self.paths[0] if self.paths else 'mjpeg'}: no frame found")
        info = parse_frame(self.read(0))
        self.w, self.h = info["w"], info["h"]

    def __len__(self) -> int:
        return len(self.entries)

    def _map(self, k: int):
        if self._maps[k] is None:
            self._maps[k] = np.memmap(self.paths[k], np.uint8, "r")
        return self._maps[k]

    def read(self, i: int) -> bytes:
        k, off, size = self.entries[i]
        return self._map(k)[off:off + size].tobytes()

    def batch(self, first: int, count: int) -> tuple:
        """(the JPEGs of frames [first, first + count) back to back as a uint8 array, offsets (count + 1,) int64)."""
        parts = [self.read(i) for i in range(first, first + count)]
        offsets = np.zeros(count + 1, np.int64)
        offsets[1:] = np.cumsum([len(b) for b in parts])
        return np.frombuffer(b"".join(parts), np.uint8), offsets


def split_mjpeg(buf) -> list:
    """(offset, size) of every JPEG in a buffer of JPEGs back to back.  Walks each frame's segments by their lengths, so that a
    complete JPEG embedded in an APPn segment (a thumbnail) does not split it; bytes between frames are skipped."""
    import re
    end_marker = re.compile(rb"\xff[^\x00\xff\xd0-\xd7]")
    size = len(buf)
    out = []
    pos = 0
    while True:
        pos = buf.find(b"\xff\xd8", pos)
        if pos < 0:
            return out
        start, p = pos, pos + 2
        ok = False
        while p + 4 <= size and buf[p] == 0xff:
            m = buf[p + 1]
            if m == 0xff:
                p += 1
                continue
            if m == 0x01 or 0xd0 <= m <= 0xd8:
                p += 2
                continue
            if m == 0xd9:
                break
            p += 2 + (buf[p + 2] << 8 | buf[p + 3])
            if m == 0xda:
                ok = True
                break
        if not ok:
            pos = start + 2
            continue
        while True:                                    # the scan, and any further one, up to EOI
            hit = end_marker.search(buf, p)
            if hit is None:
                out.append((start, size - start))      # no EOI: the file ends inside the frame
                return out
            p = hit.start()
            if buf[p + 1] == 0xd9:
                out.append((start, p + 2 - start))
                pos = p + 2
                break
            if p + 4 > size:
                out.append((start, size - start))
                return out
            p += 2 + (buf[p + 2] << 8 | buf[p + 3])


def _index_avi(path: str) -> tuple:
    """(entries (offset, size), fps) of one AVI 1.0 file: the ``movi`` list walked chunk by chunk (``idx1`` is not needed)."""
    import struct
    buf = np.memmap(path, np.uint8, "r")
    size = buf.size
    if size < 12 or buf[:4].tobytes() != b"RIFF" or buf[8:12].tobytes() != b"AVI ":
        raise NotMjpeg(f"{path}: not a RIFF 'AVI ' file")
    fps, handler, compression = 30, None, None
    entries = []
    u32 = lambda at: struct.unpack("<I", buf[at:at + 4].tobytes())[0]

    def walk(at: int, end: int, movi: bool) -> None:
        nonlocal fps, handler, compression
        while at + 8 <= end:
            cid, n = buf[at:at + 4].tobytes(), u32(at + 4)
            body = at + 8
            if cid == b"LIST" and body + 4 <= end:
                kind = buf[body:body + 4].tobytes()
                stop = body + n if 4 <= n <= end - body else end       # a size never patched in (a writer that was killed): to the end
                if kind == b"movi":
                    walk(body + 4, stop, True)
                elif kind in (b"hdrl", b"strl", b"rec "):
                    walk(body + 4, stop, movi)
                at = stop + (stop & 1)
                continue
            if n > end - body:
                if movi and cid[2:] in (b"dc", b"db"):
                    n = end - body                                    # the last chunk of a file cut short
                else:
                    return
            if movi and cid in (b"00dc", b"00db"):
                if n == 0 and entries:
                    entries.append(entries[-1])                       # a zero-length chunk repeats the previous frame
                elif n:
                    entries.append((body, n))
            elif cid == b"strh" and n >= 32 and buf[body:body + 4].tobytes() == b"vids" and handler is None:
                handler = buf[body + 4:body + 8].tobytes()
                scale, rate = u32(body + 20), u32(body + 24)
                if scale and rate:
                    fps = int(round(rate / scale))
            elif cid == b"strf" and n >= 20 and compression is None:
                compression = buf[body + 16:body + 20].tobytes()
            at = body + n + (n & 1)

    walk(12, size, False)
    if (handler or b"").upper() != b"MJPG" and (compression or b"").upper() != b"MJPG":
        raise NotMjpeg(f"{path}: the video stream is {(handler or compression or b'?').decode('ascii', 'replace')!r}, not 'MJPG'")
    return entries, fps, buf


def index_file(path) -> MjpegIndex:
    """Index a ``.avi`` (AVI 1.0 with an ``MJPG`` stream; the parts ``<stem>.part002.avi``, ... that ``video.MjpegSink`` rolls over into
    are followed) or a raw ``.mjpeg`` / ``.mjpg`` file (JPEGs back to back, 30 fps).  ``NotMjpeg``: an AVI with another codec."""
    import mmap
    import os
    path = str(path)
    stem, suffix = os.path.splitext(path)
    if suffix.lower() != ".avi":
        with open(path, "rb") as fh:
            mm = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) if os.path.getsize(path) else b""
        return MjpegIndex([path], [(0, off, n) for off, n in split_mjpeg(mm)], 30)
    paths, entries, maps, fps = [], [], [], 30
    k = 1
    while True:
        part = path if k == 1 else f"{stem}.part{k:03d}{suffix}"
        if k > 1 and not os.path.exists(part):
            break
        e, f, buf = _index_avi(part)
        if k == 1:
            fps = f
        entries += [(k - 1, off, n) for off, n in e]
        paths.append(part)
        maps.append(buf)
        k += 1
    return MjpegIndex(paths, entries, fps, maps)
