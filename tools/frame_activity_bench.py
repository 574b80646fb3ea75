#!/usr/bin/env python
"""What the court-view filter costs (csrc/frame_activity.hip, activity.scan).  GPU only.

(a) ``Engine.frame_activity`` on --frames frames of 1280 x 720 resident in HBM (with ``prev``: every frame is compared with the
    reference image and with its predecessor), alternately with ``Engine.render`` of the same frames without marks to NV12 — the
    project's measured streaming kernel (profiles/render_bench.txt) — in one session: --rounds rounds of [warm-up calls, then --reps
    calls between one pair of HIP events on the engine's stream (``pa_engine_timer_start / _stop``)] per kernel, the kernels taking
    turns.  The calls rotate over three frame sets so that a repetition does not find its frames in the 256 MB last-level cache.
    Reported per kernel: the median and the fastest round in microseconds per call, frames/s, and GB/s of the bytes it must move
    (activity: 3 bytes per pixel read — the reference image and the predecessor are cache hits by design; render: 3 read + 1.5
    written).  ``frame_activity`` is synchronous: every call ends with a 1.5 KB read-back and a host wait, which its event pair
    includes — the 4 x longer batch of the second row shows how much of a 64-frame call that is.
(b) ``activity.scan`` (reference image given) over a ``.y4m`` and a Motion-JPEG ``.avi`` of --clip-frames such frames, in frames/s by
    the host clock (conversion / decode on the GPU included), beside one ``PlayerTracker`` run of ``TrackingRunner`` over the same file.

    python tools/frame_activity_bench.py [--frames 64] [--reps 30] [--warmup 5] [--rounds 5] [--clip-frames 128] [--skip-scan]
"""
import argparse, contextlib, json, statistics, sys, tempfile, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

HBM_PEAK = 8.0e12          # bytes/s, the MI355X's HBM3E specification

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--clip-frames", type=int, default=128)
    ap.add_argument("--skip-scan", action="store_true")
    a = ap.parse_args()
    from padel_analytics_amd import activity as A, engine as E, render as R, video
    from tests import synth                                     # seeded frames (setup only)
    eng = E.default_engine(0)
    n, h, w = a.frames, a.height, a.width
    fb = h * w * 3
    print("# " + " ".join(["python", "tools/frame_activity_bench.py"] + sys.argv[1:]))
    base = synth.synthetic_frames(16, h, w, seed=1000)
    bgr = np.concatenate([np.roll(base, 7 * k, axis=2) for k in range((n + 15) // 16)])[:n]       # n distinct frames, cheaply
    ref = np.median(base, 0).astype(np.uint8)
    d_ref = eng.alloc(fb).upload(ref)

    # ---- (a) the kernels, taking turns
    SETS = 3
    long_n = 4 * n
    src = [eng.alloc(long_n * fb) for _ in range(SETS)]
    for k, s in enumerate(src):
        for j in range(4):
            s.view(j * n * fb, n * fb).upload(np.roll(bgr, k + j, axis=0))
    geom, enc = video.yuv_desc(w, h, "nv12"), video.YUV_ENC_COEFFS["bt601_limited"]
    dst = [eng.alloc(video.yuv_span(n, h, w, geom)) for _ in range(SETS)]
    marks, first = R.pack([[] for _ in range(n)])
    out = np.zeros((long_n, 3), np.uint64)
    got = eng.frame_activity(src[0].view(fb, 2 * fb), 2, h, w, d_ref, prev=src[0].view(0, fb))
    # (frames 1, 2 of set 0 against frame 0: set 0 holds bgr itself in its first quarter)
    assert np.array_equal(got, A.frame_activity_host(bgr[1:3], ref, prev=bgr[0])), got
    kernels = {
        f"frame_activity {n} frames": (lambda i: eng.frame_activity(src[i % SETS].view(fb, (n - 1) * fb), n - 1, h, w, d_ref, prev=src[i % SETS].view(0, fb), out=out),
                                       (n - 1) * fb * 1.0, n - 1),
        f"frame_activity {long_n} frames": (lambda i: eng.frame_activity(src[i % SETS].view(fb, (long_n - 1) * fb), long_n - 1, h, w, d_ref, prev=src[i % SETS].view(0, fb), out=out),
                                            (long_n - 1) * fb * 1.0, long_n - 1),
        f"render no marks -> nv12 {n} frames": (lambda i: eng.render(src[i % SETS].view(0, n * fb), n, h, w, marks, first, dst[i % SETS], out=E.RENDER_YUV420, geom=geom, enc=enc),
                                                n * h * w * 4.5, n),
    }
    times = {k: [] for k in kernels}
    for _ in range(a.rounds):
        for name, (call, moved, frames) in kernels.items():
            for i in range(a.warmup):
                call(i)
            eng.synchronize()
            eng.timer_start()
            for i in range(a.reps):
                call(i)
            times[name].append(eng.timer_stop() / a.reps)
    rate = {}
    for name, (call, moved, frames) in kernels.items():
        med, best = statistics.median(times[name]), min(times[name])
        rate[name] = moved / (med * 1e-3)
        print(json.dumps({"what": name, "us_per_call_median": round(med * 1e3, 1), "us_per_call_min": round(best * 1e3, 1), "rounds": a.rounds,
                          "reps": a.reps, "frames_per_s": round(frames / (med * 1e-3)), "GB_per_s": round(rate[name] / 1e9, 1),
                          "share_of_hbm_peak": round(rate[name] / HBM_PEAK, 3)}))
    names = list(kernels)
    print(json.dumps({"what": "frame_activity bytes/s over render bytes/s", f"{n} frames": round(rate[names[0]] / rate[names[2]], 3),
                      f"{long_n} frames": round(rate[names[1]] / rate[names[2]], 3)}))
    for b in src[1:] + dst:
        b.free()

    # ---- (b) scan over files, beside one tracker
    if not a.skip_scan:
        from padel_analytics_amd import checkpoint, detections as D, yolo_arch
        from padel_analytics_amd.trackers import PlayerTracker, TrackingRunner
        tmp = Path(tempfile.mkdtemp(prefix="frame_activity_bench_"))
        m = a.clip_frames
        sinks = {"y4m": video.Y4mSink(tmp / "clip.y4m", w, h, fps=30), "avi": video.MjpegSink(tmp / "clip.avi", w, h, fps=30, quality=90)}
        for sink in sinks.values():                                  # the files, written by the GPU: frames 0 .. m - 1 of set 0, cyclically
            buf = eng.alloc(video.yuv_span(n, h, w, sink.desc))
            done = 0
            while done < m:
                k = min(n, m - done)
                mk, fs = R.pack([[] for _ in range(k)])
                eng.render(src[0].view(0, k * fb), k, h, w, mk, fs, buf, out=E.RENDER_YUV420, geom=sink.desc, enc=sink.enc)
                sink.write_device(buf.view(0, video.yuv_span(k, h, w, sink.desc)), k)
                done += k
            sink.close()
            eng.synchronize()
            buf.free()
        checkpoint.save_checkpoint(tmp / "players.pt", yolo_arch.synth_state_dict("n", 80, None, seed=3, cls_bias=0.0), "detect", 80, None, "n", {0: "person"})
        zone = D.PolygonZone(np.array([[40, 40], [w - 40, 40], [w - 40, h - 40], [40, h - 40]]), frame_resolution_wh=(w, h))
        for kind in sinks:
            path = str(tmp / f"clip.{kind}")
            A.scan(path, ref=ref, engine=eng)                        # warm-up: the file opened, the staging allocated
            secs = []
            for _ in range(3):
                t0 = time.perf_counter()
                act = A.scan(path, ref=ref, engine=eng)
                secs.append(time.perf_counter() - t0)
            assert len(act) == m
            with contextlib.redirect_stdout(sys.stderr):
                tracker = PlayerTracker(str(tmp / "players.pt"), zone, batch_size=64)
                TrackingRunner([tracker], path, tmp / "out.mp4", engine=eng).run()         # warm-up: plan, kernels
                tracker.restart()
                runner = TrackingRunner([tracker], path, tmp / "out.mp4", engine=eng)
                runner.run()
            t = runner.timings["players_tracker"]
            tracker.model.close()
            print(json.dumps({"what": f"scan of a .{kind} file", "frames": m, "scan_frames_per_s": round(m / statistics.median(secs), 1),
                              "scan_ms_median_of_3": round(statistics.median(secs) * 1e3, 2),
                              "players_tracker_frames_per_s": round(t["frames"] / t["seconds"], 1),
                              "scan_share_of_one_tracker_run": round(statistics.median(secs) / t["seconds"], 3)}))
    src[0].free()
    d_ref.free()
