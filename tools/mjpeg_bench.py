#!/usr/bin/env python
"""What writing the annotated clip as Motion-JPEG costs (csrc/jpeg_encode.hip), alone and as the runner's render step.  GPU only.

On 64 frames of 1280 x 720 rendered with the 206-mark scene of tools/render_bench.py (I420, full-range BT.601, resident in HBM):

(a) frames 0, n / 2 and n - 1 of one ``Engine.jpeg_encode`` of the whole batch against ``mjpeg.encode_host`` (a batch of 64 is encoded
    in sub-batches inside the call, which no test is large enough to reach), and the bytes per frame;
(b) ``pa_jpeg_encode`` with a destination of 0 bytes — the encode, offsets and gather kernels, the read-back of the sizes and the
    host's turnaround between sub-batches, but no download of the frames — between one pair of HIP events, per call;
(c) the whole call (kernels + download of the compressed bytes) with a host clock;
(d) ``TrackingRunner``'s render step on the same clip and marks, end to end, with ``render="out.avi"`` beside ``render="out.y4m"``:
    the two sinks alternately in one session, host clock, one untimed pass each first;
(e) the parts of that step alone, host clock: building and packing the marks, the render, writing the file.

    python tools/mjpeg_bench.py [--frames 64] [--reps 20] [--warmup 3] [--passes 5] [--quality 90] [--kernel-only]

``--kernel-only`` runs (b) with few repetitions and nothing else: the run to put under ``rocprofv3 --kernel-trace --stats``.
"""
import argparse, contextlib, json, statistics, sys, tempfile, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    from render_bench import Joints, Stored, scene
    from padel_analytics_amd import engine as E, mjpeg, render as R, video
    from padel_analytics_amd.trackers import TrackingRunner
    from padel_analytics_amd.trackers.ball_tracker import Ball
    from padel_analytics_amd.trackers.keypoints_tracker import Keypoints
    from padel_analytics_amd.trackers.players_tracker import Players
    from tests import synth                                     # seeded frames (setup only)
    eng = E.default_engine(0)
    n, h, w, q = a.frames, a.height, a.width, a.quality
    print("# " + " ".join(["python", "tools/mjpeg_bench.py"] + sys.argv[1:]))
    bgr = synth.synthetic_frames(n, h, w, seed=1000)
    info = video.VideoInfo(w, h, 30, n)
    scenes = [scene(i, w, h) for i in range(n)]
    trackers = [Stored("players_tracker", [s[0] for s in scenes], {"video_info": info, "annotator": "rectangle_bounding_box", "show_confidence": True}, Players),
                Stored("players_keypoints_tracker", [s[1] for s in scenes]), Stored("joints", [Joints(s[1]) for s in scenes]),
                Stored("ball_tracker", [s[2] for s in scenes], kind=Ball), Stored("keypoints_tracker", [s[3] for s in scenes], kind=Keypoints)]
    clip = video.DeviceClip(eng, bgr)
    tmp = Path(tempfile.mkdtemp(prefix="mjpeg_bench_"))
    runners = {name: TrackingRunner(trackers, clip, tmp / "out.mp4", render=tmp / name, engine=eng, render_quality=q) for name in ("out.avi", "out.y4m")}
    marks, first = R.pack([runners["out.avi"].frame_marks(i) for i in range(n)])
    geom = video.yuv_desc(w, h, "i420", "bt601", "full")
    yuv = eng.alloc(video.yuv_span(n, h, w, geom))
    eng.render(clip.buffer, n, h, w, marks, first, yuv, out=E.RENDER_YUV420, geom=geom, enc=video.YUV_ENC_COEFFS["bt601_full"])
    print(json.dumps({"what": "scene", "marks_per_frame": int(first[1]), "frames": n, "h": h, "w": w, "quality": q,
                      "raw_yuv420_bytes_per_frame": w * h * 3 // 2, "slot_bytes_per_interval": E.jpeg_interval_bytes(w)}))

    nothing = np.empty(0, np.uint8)

    def kernels_only():
        try:
            eng.jpeg_encode(yuv, n, h, w, geom, q, out=nothing)
        except E.EngineError as e:
            return e.needed
    for _ in range(a.warmup):
        kernels_only()
    eng.synchronize()
    each = []
    for _ in range(3 if a.kernel_only else a.reps):
        eng.timer_start()
        total = kernels_only()
        each.append(eng.timer_stop())
    print(json.dumps({"what": "pa_jpeg_encode with no destination: encode + offsets + gather kernels, size read-backs, no frame download; HIP events per call",
                      "ms_median_min_max": [round(statistics.median(each), 3), round(min(each), 3), round(max(each), 3)],
                      "frames_per_s": round(n / (statistics.median(each) * 1e-3)), "bytes_total": int(total), "bytes_per_frame": int(total) // n}))
    if a.kernel_only:
        sys.exit(0)

    # ---- (a) the bytes, checked and counted
    data, offsets = eng.jpeg_encode(yuv, n, h, w, geom, q)
    raw = yuv.download(np.empty(yuv.nbytes, np.uint8))
    for i in sorted({0, n // 2, n - 1}):
        want, _ = mjpeg.encode_host(raw[i * geom["frame_stride"]:][:video.yuv_span(1, h, w, geom)], 1, h, w, geom, q)
        assert np.array_equal(data[offsets[i]:offsets[i + 1]], want), f"frame {i} differs from mjpeg.encode_host"
    sizes = np.diff(offsets)
    print(json.dumps({"what": "Engine.jpeg_encode of the batch: frames 0, n / 2, n - 1 equal mjpeg.encode_host", "bytes_per_frame_mean_min_max":
                      [int(sizes.mean()), int(sizes.min()), int(sizes.max())], "share_of_raw_yuv420": round(float(sizes.mean()) / (w * h * 1.5), 4)}))

    # ---- (c) the whole call
    out = np.empty(int(offsets[-1]) * 2, np.uint8)
    secs = []
    for k in range(a.warmup + a.reps):
        eng.synchronize()
        t0 = time.perf_counter()
        eng.jpeg_encode(yuv, n, h, w, geom, q, out=out)
        secs.append(time.perf_counter() - t0)
    secs = secs[a.warmup:]
    print(json.dumps({"what": "Engine.jpeg_encode: kernels + download of the compressed frames, host clock per call",
                      "ms_median_min_max": [round(1e3 * statistics.median(secs), 3), round(1e3 * min(secs), 3), round(1e3 * max(secs), 3)],
                      "frames_per_s": round(n / statistics.median(secs))}))

    # ---- (d) the runner's render step, the two sinks alternately
    secs = {name: [] for name in runners}
    sizes = {}
    with contextlib.redirect_stdout(sys.stderr):
        for k in range(a.passes + 1):                               # one untimed pass each first
            for name, r in runners.items():
                eng.synchronize()
                t0 = time.perf_counter()
                r.draw_and_collect_data()
                secs[name].append(time.perf_counter() - t0)
                sizes[name] = (tmp / name).stat().st_size
                (tmp / name).unlink()
    for name in runners:
        s = secs[name][1:]
        med = statistics.median(s)
        print(json.dumps({"what": f"TrackingRunner render step, render={name!r} (host clock; passes alternate between the sinks)", "frames": n,
                          "seconds_median": round(med, 4), "seconds_passes": [round(v, 4) for v in s], "frames_per_s": round(n / med, 1),
                          "file_bytes": sizes[name], "MB_per_s_written": round(sizes[name] / med / 1e6, 1)}))
    # ---- (e) where the .avi step's time goes: its host parts alone (host clock, median of the passes)
    r = runners["out.avi"]
    parts = {"marks: frame_marks + render.pack of the batch": [], "render: Engine.render + synchronize": [], "write: MjpegSink.write_jpegs + close": []}
    for k in range(a.passes + 1):
        t0 = time.perf_counter()
        packed = R.pack([r.frame_marks(i) for i in range(n)])
        t1 = time.perf_counter()
        eng.render(clip.buffer, n, h, w, *packed, yuv, out=E.RENDER_YUV420, geom=geom, enc=video.YUV_ENC_COEFFS["bt601_full"])
        eng.synchronize()
        t2 = time.perf_counter()
        sink = video.MjpegSink(tmp / "parts.avi", w, h, quality=q)
        t3 = time.perf_counter()
        sink.write_jpegs(data, offsets)
        sink.close()
        t4 = time.perf_counter()
        for key, v in zip(parts, (t1 - t0, t2 - t1, t4 - t3)):
            parts[key].append(v)
        (tmp / "parts.avi").unlink()
    print(json.dumps({"what": "the parts of the .avi render step alone, ms per batch of %d frames (host clock, median of %d passes after one untimed)" % (n, a.passes),
                      **{key: round(1e3 * statistics.median(v[1:]), 3) for key, v in parts.items()}}))
    yuv.free()
    clip.free()
