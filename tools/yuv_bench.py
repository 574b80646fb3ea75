#!/usr/bin/env python
"""What the YUV 4:2:0 -> BGR conversion (csrc/yuv_convert.hip) costs, alone and beside the step it feeds.  GPU only.

(a) the kernel alone on 64 frames of 1280 x 720, per layout (NV12, I420) and per path (vector: aligned tight frames; byte: the
    same frames behind a source pointer moved by one byte), timed with HIP events on the engine's stream: microseconds and GB/s
    of the 4.5 bytes per pixel it must move (1.5 read, 3 written).  Warm-up calls first, then one event pair per call; the median
    and the spread are reported.  The calls rotate over three source / destination sets (265 MB each), so that a
    repetition does not find its bytes in the 256 MB last-level cache.
(b) frames/s of one model (the players detector, YOLOv8n, seeded synthetic checkpoint) through TrackingRunner over the same 64
    frames presented --passes times, for four sources: a page-locked BGR ArrayClip, a page-locked NV12 YuvClip, a
    DeviceYuvClip, a BGR DeviceClip.  One untimed pass each, then --rounds timed rounds that alternate the four; a host clock
    around runs that end in a device synchronise.

    python tools/yuv_bench.py [--frames 64] [--reps 30] [--warmup 5] [--passes 16] [--rounds 3] [--skip-runner]
"""
import argparse, json, mmap, statistics, sys, tempfile, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def anon_copy(a: np.ndarray) -> np.ndarray:
    """``a``'s bytes in an anonymous private mapping (page-aligned, never malloc's heap): memory to page-lock."""
    mm = mmap.mmap(-1, a.nbytes, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS, prot=mmap.PROT_READ | mmap.PROT_WRITE)
    out = np.frombuffer(mm, np.uint8)[:a.nbytes]
    out[:] = a.reshape(-1).view(np.uint8)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--passes", type=int, default=16, help="(b): times the clip is presented per timed run")
    ap.add_argument("--rounds", type=int, default=3, help="(b): timed rounds, each running the four sources in turn")
    ap.add_argument("--skip-runner", action="store_true")
    a = ap.parse_args()
    from padel_analytics_amd import checkpoint, engine as E, video, yolo_arch
    from padel_analytics_amd.trackers import PlayerTracker, TrackingRunner
    from tests import synth, yuv_ref as Y                     # seeded frames and the test encoder (setup only)
    eng = E.default_engine(0)
    n, h, w = a.frames, a.height, a.width
    print("# " + " ".join(["python", "tools/yuv_bench.py"] + sys.argv[1:]))
    bgr = synth.synthetic_frames(n, h, w, seed=1000)
    moved = n * h * w * 4.5

    # ---- (a) the kernel alone
    SETS = 3
    for layout in ("nv12", "i420"):
        raw, g = Y.bgr_to_yuv420(bgr, layout)
        desc = video.yuv_desc(w, h, layout)
        src = [eng.alloc(raw.size + 4).upload(np.concatenate([np.zeros(1, np.uint8), raw])) for _ in range(SETS)]      # frames at byte 1 ...
        src_al = [eng.alloc(raw.size).upload(raw) for _ in range(SETS)]                                               # ... and at byte 0
        dst = [eng.alloc(n * h * w * 3) for _ in range(SETS)]
        for path, bufs in (("vector", src_al), ("byte", [b.view(1, raw.size) for b in src])):
            for i in range(a.warmup):
                eng.yuv420_to_bgr(bufs[i % SETS], n, h, w, desc, dst[i % SETS])
            eng.synchronize()
            assert eng.yuv_last_path() == (E.YUV_PATH_VECTOR if path == "vector" else E.YUV_PATH_BYTE)
            ms = []
            for i in range(a.reps):
                eng.timer_start()
                eng.yuv420_to_bgr(bufs[i % SETS], n, h, w, desc, dst[i % SETS])
                ms.append(eng.timer_stop())
            med = statistics.median(ms)
            print(json.dumps({"what": "kernel alone, HIP events", "layout": layout, "path": path, "frames": n, "h": h, "w": w,
                              "reps": a.reps, "warmup": a.warmup, "us_median": round(1e3 * med, 1),
                              "us_min_max": [round(1e3 * min(ms), 1), round(1e3 * max(ms), 1)],
                              "GB_per_s_of_4.5_B_per_px": round(moved / (med * 1e-3) / 1e9, 1), "bytes_moved": int(moved)}))
        for b in src + src_al + dst:
            b.free()

    # ---- (b) one model through the runner, four frame sources
    if not a.skip_runner:
        tmp = Path(tempfile.mkdtemp(prefix="yuv_bench_"))
        checkpoint.save_checkpoint(tmp / "players.pt", yolo_arch.synth_state_dict("n", 80, None, seed=3, cls_bias=0.5), "detect", 80, None,
                                   "n", {0: "person"})
        tracker = PlayerTracker(str(tmp / "players.pt"), None, batch_size=n)
        raw, g = Y.bgr_to_yuv420(bgr, "nv12")
        bgr_ref = Y.convert(raw, n, h, w, g, Y.COEFFS["bt601_limited"])            # every source shows the model the same pixels
        K = a.passes
        pinned_bgr = anon_copy(bgr_ref).reshape(bgr_ref.shape)
        sources = {
            "pinned BGR ArrayClip": video.ArrayClip(pinned_bgr, repeat=K).pin(eng),
            "pinned NV12 YuvClip": video.YuvClip(anon_copy(raw), w, h, repeat=K, engine=eng).pin(eng),
            "DeviceYuvClip (NV12 in HBM)": video.DeviceYuvClip(eng, raw, w, h, repeat=K),
            "BGR DeviceClip (in HBM)": video.DeviceClip(eng, bgr_ref, repeat=K),
        }

        def run(source, passes):
            r = TrackingRunner([tracker], source, tmp / "out.mp4", start=0, end=passes * n)
            r.restart()
            eng.synchronize()
            t0 = time.perf_counter()
            r.run()
            eng.synchronize()
            return time.perf_counter() - t0

        import contextlib
        with contextlib.redirect_stdout(sys.stderr):
            for s in sources.values():
                run(s, 1)
            rates = {k: [] for k in sources}
            for _ in range(a.rounds):
                for k, s in sources.items():
                    rates[k].append(K * n / run(s, K))
        for k, v in rates.items():
            print(json.dumps({"what": "players detector (YOLOv8n @640, batch %d) through TrackingRunner" % n, "source": k,
                              "frames_per_run": K * n, "frames_per_s_median": round(statistics.median(v), 1),
                              "frames_per_s_rounds": [round(x, 1) for x in v],
                              "host_bytes_per_frame": {"pinned BGR ArrayClip": h * w * 3, "pinned NV12 YuvClip": h * w * 3 // 2}.get(k, 0)}))
        sources["pinned BGR ArrayClip"].unpin()
        sources["pinned NV12 YuvClip"].unpin()
        for k in ("pinned NV12 YuvClip", "DeviceYuvClip (NV12 in HBM)", "BGR DeviceClip (in HBM)"):
            sources[k].free()
        tracker.model.close()
