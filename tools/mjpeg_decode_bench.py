#!/usr/bin/env python
"""What reading a Motion-JPEG clip costs (csrc/jpeg_decode.hip), alone and as the runner's source.  GPU only.

64 frames of 1280 x 720 (seeded synthetic frames), encoded by the project's own writer at quality 90 (``Engine.jpeg_encode``: one
restart interval per MCU row), and the same frames twice more: with the writer's coefficients and tables but NO restart markers (the
twin's entropy coder over the whole frame as one interval), and by Pillow with ``optimize=True`` (no restart markers, per-frame
Huffman tables).  For each of the three:

(a) frames 0, n / 2 and n - 1 of one ``Engine.jpeg_decode`` of the whole batch against ``mjpeg.decode_host``;
(b) the stages of the call apart, with profiling on: reading the markers (host clock), the upload of the compressed bytes and tables,
    the entropy pass, the IDCT pass and the colour pass (HIP events), per call of n frames;
(c) the whole call with a host clock, profiling off: frames per second of the decode.

Then, in the same session:

(d) ``Engine.yuv420_to_bgr`` of the same frames as raw I420 in host memory (what ``YuvClip`` does per batch: upload + convert);
(e) ``TrackingRunner`` with a player tracker (synthetic weights) over the ``.avi`` beside the same run over the ``.y4m`` of the same
    frames, by path, the two sources alternately, host clock, one untimed pass each first.

The split entropy path (csrc/jpeg_entropy_split.h: an interval of ``min_bytes`` and more is decoded by a workgroup, its bytes cut into
subsequences of ``sub_bytes``), on Pillow's encoding of the same frames with the default tables (what ``ffmpeg -c:v mjpeg`` and Pillow
write), sections f, g, h:

(f) the stages and the whole call of the stream without restart markers, ``jpeg_decode_set_split(-1)`` (every interval on the
    one-wave kernel: the behaviour before the split path) and the default alternately, call by call, with the rounds the kernel reports;
(g) the sweep behind the two defaults: restart intervals of 1, 3 and 9 MCU rows and none (Pillow's ``restart_marker_rows``), each on
    the one-wave kernel and split with ``sub_bytes`` 32 .. 1024: the entropy pass per call, the rounds;
(h) the runner as in (e) over three sources alternately: the ``.avi`` without restart markers, the writer's ``.avi``, the ``.y4m``.

    python tools/mjpeg_decode_bench.py [--frames 64] [--reps 10] [--warmup 2] [--passes 3] [--quality 90] [--sections abcdefgh]
"""
import argparse, contextlib, io, json, statistics, sys, tempfile, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def no_restart(mjpeg, y, cb, cr, quality) -> bytes:
    """The writer's frame as ONE interval: its coefficients and tables, no DRI segment, no RSTm."""
    h, w = y.shape
    head = mjpeg.frame_header(h, w, quality)
    dri = head.index(b"\xff\xdd\x00\x04")
    z = mjpeg.frame_coefficients(y, cb, cr, quality)
    return head[:dri] + head[dri + 6:] + mjpeg.pack_interval(*mjpeg.interval_entries(z.reshape(-1, 6, 64))) + b"\xff\xd9"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--sections", default="abcdefgh", help="which of the sections above run (a, b, c go together)")
    ap.add_argument("--dump", default=None, help="write the frames without restart markers of (f) there as records of (uint32 length, JPEG): "
                                                 "the input of tests/jpeg_split_main.cpp, which counts the symbols the rounds decode")
    a = ap.parse_args()
    from PIL import Image
    from padel_analytics_amd import checkpoint, detections as D, engine as E, mjpeg, video, yolo_arch
    from padel_analytics_amd.trackers import PlayerTracker, TrackingRunner
    from tests import synth                                     # seeded frames (setup only)
    eng = E.default_engine(0)
    n, h, w, q = a.frames, a.height, a.width, a.quality
    print("# " + " ".join(["python", "tools/mjpeg_decode_bench.py"] + sys.argv[1:]))
    bgr = synth.synthetic_frames(n, h, w, seed=1000)
    geom = video.yuv_desc(w, h, "i420", "bt601", "full")
    raw = video.bgr_to_yuv420_host(bgr, geom, video.YUV_ENC_COEFFS["bt601_full"])
    yuv = eng.alloc(raw.size)
    yuv.upload(raw)
    data, offsets = eng.jpeg_encode(yuv, n, h, w, geom, q)
    yuv.free()
    rows = [data[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in range(n)]
    abc = bool(set("abc") & set(a.sections))
    t0 = time.perf_counter()
    flat = [no_restart(mjpeg, *mjpeg.planes(raw, i, h, w, geom), q) for i in range(n)] if abc else []
    t1 = time.perf_counter()
    dst = eng.alloc(n * h * w * 3)
    eng.jpeg_decode(data, offsets, dst)
    decoded = dst.download(np.empty((n, h, w, 3), np.uint8))

    def pillow(**kw) -> list:
        res = []
        for i in range(n):
            out = io.BytesIO()
            Image.fromarray(decoded[i, ..., ::-1]).save(out, "JPEG", quality=q, subsampling=2, **kw)
            res.append(out.getvalue())
        return res

    def packed(jpegs: list) -> tuple:
        return np.frombuffer(b"".join(jpegs), np.uint8), np.cumsum([0] + [len(j) for j in jpegs]).astype(np.int64)

    def same_as_host(jpegs: list, name: str) -> None:
        """One decode of the batch: every status zero, frames 0, n / 2, n - 1 equal to the twin's."""
        status = eng.jpeg_decode(*packed(jpegs), dst)
        got = dst.download(np.empty((n, h, w, 3), np.uint8))
        assert not status.any(), status
        for i in sorted({0, n // 2, n - 1}):
            if jpegs[i] not in twin:
                twin[jpegs[i]] = mjpeg.decode_frame(jpegs[i])[0]
            assert np.array_equal(got[i], twin[jpegs[i]]), f"{name}: frame {i} differs from mjpeg.decode_host"

    twin = {}                                                   # JPEG -> the twin's pixels: every frame compared is decoded there once
    pil = pillow(optimize=True) if abc else []
    print(json.dumps({"what": "setup", "frames": n, "h": h, "w": w, "quality": q, "bgr_bytes_per_frame": h * w * 3,
                      "seconds_to_build_the_no_restart_streams_on_the_host": round(t1 - t0, 1)}))

    streams = {"restart per MCU row (the writer)": rows, "no restart markers (the writer's coefficients, one interval)": flat,
               "Pillow optimize=True (no restart markers, own tables)": pil}
    for name, jpegs in (streams.items() if abc else ()):
        blob = np.frombuffer(b"".join(jpegs), np.uint8)
        offs = np.cumsum([0] + [len(j) for j in jpegs]).astype(np.int64)
        status = eng.jpeg_decode(blob, offs, dst)
        got = dst.download(np.empty((n, h, w, 3), np.uint8))
        assert not status.any(), status
        for i in sorted({0, n // 2, n - 1}):
            assert np.array_equal(got[i], mjpeg.decode_frame(jpegs[i])[0]), f"{name}: frame {i} differs from mjpeg.decode_host"
        if jpegs is flat:
            assert np.array_equal(got, decoded), "the no-restart streams do not decode to the writer's pixels"
        info = mjpeg.parse_frame(jpegs[0])
        eng.set_profiling(True)
        stages = []
        for k in range(a.warmup + a.reps):
            eng.jpeg_decode(blob, offs, dst)
            stages.append(eng.jpeg_decode_last_times())
        eng.set_profiling(False)
        stages = stages[a.warmup:]
        med = {key: round(statistics.median(s[key] for s in stages), 3) for key in stages[0]}
        secs = []
        for k in range(a.warmup + a.reps):
            eng.synchronize()
            t0 = time.perf_counter()
            eng.jpeg_decode(blob, offs, dst)
            secs.append(time.perf_counter() - t0)
        secs = secs[a.warmup:]
        print(json.dumps({"what": f"Engine.jpeg_decode of {n} frames: {name}; frames 0, n / 2, n - 1 equal mjpeg.decode_host",
                          "intervals_per_frame": info["n_intervals"], "bytes_per_frame_mean": int(blob.size // n),
                          "share_of_bgr": round(blob.size / n / (h * w * 3), 4), "ms_per_call_by_stage_median": med,
                          "ms_per_call_host_clock_median_min_max": [round(1e3 * statistics.median(secs), 3), round(1e3 * min(secs), 3),
                                                                    round(1e3 * max(secs), 3)],
                          "frames_per_s": round(n / statistics.median(secs))}))

    # ---- (f) the stream without restart markers: every interval on the one-wave kernel and the default, call by call
    med3 = lambda v: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)]
    plain = pillow() if set("fgh") & set(a.sections) else []
    if a.dump and plain:
        import struct
        Path(a.dump).write_bytes(b"".join(struct.pack("<I", len(j)) + j for j in plain))
    if "f" in a.sections:
        for label, jpegs in (("Pillow's default tables", plain), ("Pillow optimize=True", pillow(optimize=True))):
            blob, offs = packed(jpegs)
            modes = {"set_split(-1): one wave per interval": (-1, 0), "set_split(0, 0): the defaults": (0, 0)}
            stage = {m: [] for m in modes}
            whole = {m: [] for m in modes}
            report = {}
            for m, args in modes.items():
                eng.jpeg_decode_set_split(*args)
                same_as_host(jpegs, m)
            for timed in (True, False):
                eng.set_profiling(timed)
                for k in range(a.warmup + a.reps):
                    for m, args in modes.items():
                        eng.jpeg_decode_set_split(*args)
                        eng.synchronize()
                        t0 = time.perf_counter()
                        eng.jpeg_decode(blob, offs, dst)
                        t1 = time.perf_counter()
                        if k >= a.warmup:
                            if timed:
                                stage[m].append(eng.jpeg_decode_last_times())
                                report[m] = eng.jpeg_decode_last_split()
                            else:
                                whole[m].append(1e3 * (t1 - t0))
            eng.set_profiling(False)
            eng.jpeg_decode_set_split(0, 0)
            for m in modes:
                print(json.dumps({"what": f"Engine.jpeg_decode of {n} frames, {label}, no restart markers; {m} (the two alternate call by call)",
                                  "bytes_per_frame_mean": int(blob.size // n), "last_split": report[m],
                                  "ms_per_call_by_stage_median": {key: round(statistics.median(s[key] for s in stage[m]), 3) for key in stage[m][0]},
                                  "entropy_ms_median_min_max": med3([s["entropy"] for s in stage[m]]),
                                  "ms_per_call_host_clock_median_min_max": med3(whole[m]), "frames_per_s": round(n / statistics.median(whole[m]) * 1e3)}))

    # ---- (g) the sweep: interval length x sub_bytes
    if "g" in a.sections:
        eng.set_profiling(True)
        for rows_per_interval in (1, 3, 9, None):
            jpegs = plain if rows_per_interval is None else pillow(restart_marker_rows=rows_per_interval)
            blob, offs = packed(jpegs)
            info = mjpeg.parse_frame(jpegs[0])
            lens = [e - b for j in jpegs for b, e, _, _ in mjpeg.parse_frame(j)["intervals"]]
            row = {"what": f"entropy pass of {n} frames, restart interval = {rows_per_interval or 'none'} MCU rows", "intervals_per_frame": info["n_intervals"],
                   "interval_bytes_mean_min_max": [int(statistics.mean(lens)), min(lens), max(lens)], "entropy_ms_median_min_max": {}, "rounds": {}}
            for sub_bytes in (None, 32, 64, 128, 256, 512, 1024):
                eng.jpeg_decode_set_split(*((-1, 0) if sub_bytes is None else (1, sub_bytes)))
                same_as_host(jpegs, str((rows_per_interval, sub_bytes)))
                ms = []
                for k in range(a.warmup + a.reps):
                    eng.jpeg_decode(blob, offs, dst)
                    ms.append(eng.jpeg_decode_last_times()["entropy"])
                key = "one wave" if sub_bytes is None else f"split {sub_bytes}"
                row["entropy_ms_median_min_max"][key] = med3(ms[a.warmup:])
                row["rounds"][key] = eng.jpeg_decode_last_split()["rounds"]
            print(json.dumps(row))
        eng.set_profiling(False)
        eng.jpeg_decode_set_split(0, 0)

    # ---- (d) the same frames as raw I420 in host memory: upload + convert
    secs = []
    for k in range(a.warmup + a.reps if "d" in a.sections else 0):
        eng.synchronize()
        t0 = time.perf_counter()
        eng.yuv420_to_bgr(raw, n, h, w, geom, dst)
        eng.synchronize()
        secs.append(time.perf_counter() - t0)
    secs = secs[a.warmup:]
    if secs:
        print(json.dumps({"what": f"Engine.yuv420_to_bgr of the same {n} frames as raw I420 in pageable host memory (upload + convert), host clock",
                          "bytes_per_frame": raw.size // n, "ms_per_call_median_min_max": [round(1e3 * statistics.median(secs), 3), round(1e3 * min(secs), 3),
                                                                                          round(1e3 * max(secs), 3)],
                          "frames_per_s": round(n / statistics.median(secs))}))
    dst.free()

    # ---- (e) the runner from the .avi beside the runner from the .y4m
    tmp = Path(tempfile.mkdtemp(prefix="mjpeg_decode_bench_"))
    with video.MjpegSink(tmp / "clip.avi", w, h, quality=q) as sink:
        sink.write_jpegs(data, offsets)
    with video.Y4mSink(tmp / "clip.y4m", w, h, range="full") as sink:
        sink.write_host(raw, n)
    checkpoint.save_checkpoint(tmp / "players.pt", yolo_arch.synth_state_dict("n", 80, None, seed=3, cls_bias=0.5), "detect", 80, None, "n",
                               {0: "person"})
    zone = D.PolygonZone(np.array([[40, 40], [w - 40, 40], [w - 40, h - 40], [40, h - 40]]), frame_resolution_wh=(w, h))
    tracker = PlayerTracker(str(tmp / "players.pt"), zone, batch_size=16)
    secs = {"clip.avi": [], "clip.y4m": []} if "e" in a.sections else {}
    if "h" in a.sections:
        with video.MjpegSink(tmp / "plain.avi", w, h, quality=q) as sink:
            sink.write_jpegs(*packed(plain))
        secs = {"plain.avi": [], "clip.avi": [], "clip.y4m": []}
    with contextlib.redirect_stdout(sys.stderr):
        for k in range(a.passes + 1):                               # one untimed pass each first
            for name in secs:
                r = TrackingRunner([tracker], str(tmp / name), tmp / "out.mp4", engine=eng)
                r.restart()
                eng.synchronize()
                t0 = time.perf_counter()
                r.run()
                eng.synchronize()
                secs[name].append(time.perf_counter() - t0)
                assert len(tracker) == n
    for name, s in secs.items():
        s = s[1:]
        print(json.dumps({"what": f"TrackingRunner, one player tracker (YOLOv8n, synthetic weights, batch 16), source {name!r} by path "
                                  f"(host clock; passes alternate between the sources)", "frames": n, "file_bytes": (tmp / name).stat().st_size,
                          "seconds_median": round(statistics.median(s), 4), "seconds_passes": [round(v, 4) for v in s],
                          "frames_per_s": round(n / statistics.median(s), 1)}))
    for name in secs:
        if name.endswith(".avi"):
            clip = video._open_mjpeg(str(tmp / name))
            print(json.dumps({"what": f"the source {name!r} inside those runs (plain.avi: Pillow's frames without restart markers; clip.avi: the "
                                      f"writer's, one interval per MCU row)", "decodes": clip.decodes, "corrupt_frames": len(clip.corrupt)}))
