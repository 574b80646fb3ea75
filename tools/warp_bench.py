#!/usr/bin/env python
"""What the top-down view costs (csrc/warp.hip, TrackingRunner(topdown=)).  GPU only.  One session, the legs taking turns.

(a) ``Engine.warp`` of --frames frames of 1280 x 720 resident in HBM into the default canvas (624 x 1104) through a plausible court
    homography, beside ``Engine.render`` of the same frames without marks to I420 — the project's streaming yardstick: --rounds rounds
    of [warm-up calls, then --reps calls between one pair of HIP events on the engine's stream (``pa_engine_timer_start / _stop``)]
    per leg.  Reported: the median and the fastest round in microseconds per call, frames/s, and GB/s of the bytes the call must move
    (warp: the canvas written plus the source read once; render: the source read plus the 4:2:0 planes written).
(b) The runner's render step (``draw_and_collect_data``) over a ``.y4m`` file of --clip-frames such frames (read, uploaded and converted to
    BGR on the GPU once per walk), with stored results (fixed
    court keypoints, four players, a ball: tests/court_script.py), writing Motion-JPEG: ``topdown="x.avi"`` alone, ``render="y.avi"``
    alone, and both, --step-rounds rounds of the three by turns, in seconds by the host clock (the step ends in a synchronise).
    Reported: the medians, and what the shared walk saves: (alone + alone) - both.
(c) --render-only: leg "render alone" of (b) by itself, for a run against another build of the library (PADEL_LIB): the parent
    commit's, by turns with this one's, in fresh processes.

    python tools/warp_bench.py [--frames 64] [--reps 20] [--warmup 3] [--rounds 5] [--clip-frames 256] [--step-rounds 3] [--render-only]
"""
import argparse, contextlib, json, statistics, sys, tempfile, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--clip-frames", type=int, default=256)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--render-only", action="store_true")
    a = ap.parse_args()
    from padel_analytics_amd import engine as E, render as R, topdown as T, video
    from padel_analytics_amd.trackers import TrackingRunner
    from tests import court_script as CS, synth                 # seeded frames and results (setup only)
    eng = E.default_engine(0)
    n, h, w = a.frames, 720, 1280
    fb = h * w * 3
    print("# " + " ".join(["python", "tools/warp_bench.py"] + sys.argv[1:]) + f"   (library: {E.lib_path().name})")
    base = synth.synthetic_frames(16, h, w, seed=1000)
    bgr = np.concatenate([np.roll(base, 7 * k, axis=2) for k in range((n + 15) // 16)])[:n]       # n distinct frames, cheaply
    court = CS.court_for(w, h)
    H = CS.true_homography(court, np.random.default_rng(0))

    # ---- (a) the kernel beside the renderer
    if not a.render_only:
        view = T.TopDownView(court)
        m, valid = view.matrices([CS.PC.FrameProjection(H, None, None)] * n)
        src = eng.alloc(n * fb).upload(bgr)
        canvas = eng.alloc(n * view.h * view.w * 3)
        geom, enc = video.yuv_desc(w, h, "i420"), video.YUV_ENC_COEFFS["bt601_limited"]
        yuv = eng.alloc(video.yuv_span(n, h, w, geom))
        none, first = R.pack([[] for _ in range(n)])
        eng.warp(src, 2, h, w, m[:2], valid[:2], canvas, view.h, view.w, fill=view.fill)
        got = canvas.download(np.empty(2 * view.h * view.w * 3, np.uint8)).reshape(2, view.h, view.w, 3)
        assert np.array_equal(got, T.warp_host(bgr[:2], m[:2], valid[:2], view.h, view.w, view.fill)), "the kernel differs from warp_host"
        legs = {"warp": lambda: eng.warp(src, n, h, w, m, valid, canvas, view.h, view.w, fill=view.fill),
                "render": lambda: eng.render(src, n, h, w, none, first, yuv, out=E.RENDER_YUV420, geom=geom, enc=enc)}
        moved = {"warp": n * (fb + view.h * view.w * 3), "render": n * (fb + h * w * 3 // 2)}
        times = {k: [] for k in legs}
        for _ in range(a.rounds):
            for name, call in legs.items():
                for _ in range(a.warmup):
                    call()
                eng.synchronize()
                eng.timer_start()
                for _ in range(a.reps):
                    call()
                times[name].append(eng.timer_stop() / a.reps)
        for name in legs:
            med, best = statistics.median(times[name]), min(times[name])
            print(json.dumps({"what": f"Engine.{name} of {n} frames 1280x720" + (f" -> {view.w}x{view.h}, path {eng.warp_last_path()}" if name == "warp" else " -> I420, no marks"),
                              "us_per_call_median": round(med * 1e3, 1), "us_per_call_min": round(best * 1e3, 1), "rounds": a.rounds, "reps": a.reps,
                              "frames_per_s": round(n / (med * 1e-3)), "GB_per_s_of_bytes_that_must_move": round(moved[name] / (med * 1e-3) / 1e9, 1)}))
        for b in (src, canvas, yuv):
            b.free()

    # ---- (b) / (c) the runner's step
    mclip = a.clip_frames
    kps, players, balls = CS.scripted_clip(mclip, same_keypoints=True)
    tmp = Path(tempfile.mkdtemp(prefix="warp_bench_"))
    sink = video.Y4mSink(tmp / "clip.y4m", w, h, fps=30)            # the file, written by the GPU: the n frames, cyclically
    src = eng.alloc(n * fb).upload(bgr)
    buf = eng.alloc(video.yuv_span(n, h, w, sink.desc))
    done = 0
    while done < mclip:
        k = min(n, mclip - done)
        mk, fs = R.pack([[] for _ in range(k)])
        eng.render(src.view(0, k * fb), k, h, w, mk, fs, buf, out=E.RENDER_YUV420, geom=sink.desc, enc=sink.enc)
        sink.write_device(buf.view(0, video.yuv_span(k, h, w, sink.desc)), k)
        done += k
    sink.close()
    eng.synchronize()
    src.free()
    buf.free()
    clip = str(tmp / "clip.y4m")

    def step(**kw):
        runner = TrackingRunner(CS.stub_trackers(kps, players, balls, fixed=kps[0]), clip, tmp / "out.mp4", engine=eng, end=mclip, **kw)
        with contextlib.redirect_stdout(sys.stderr):
            t0 = time.perf_counter()
            runner.draw_and_collect_data()
            eng.synchronize()
            return time.perf_counter() - t0

    configs = {"render alone": dict(render=tmp / "y.avi")}
    if not a.render_only:
        configs = {"topdown alone": dict(topdown=tmp / "x.avi"), **configs, "both": dict(topdown=tmp / "x.avi", render=tmp / "y.avi")}
    for kw in configs.values():
        step(**kw)                                               # warm-up: kernels, the sinks' buffers
    secs = {k: [] for k in configs}
    for _ in range(a.step_rounds):
        for name, kw in configs.items():
            secs[name].append(step(**kw))
    med = {k: statistics.median(v) for k, v in secs.items()}
    row = {"what": f"the runner's render step, {mclip} frames 1280x720 from a .y4m file, Motion-JPEG out", "rounds": a.step_rounds}
    for k in configs:
        row[k.replace(" ", "_") + "_s"] = round(med[k], 4)
        row[k.replace(" ", "_") + "_s_all"] = [round(v, 4) for v in secs[k]]
        row[k.replace(" ", "_") + "_frames_per_s"] = round(mclip / med[k], 1)
    if not a.render_only:
        row["alone_plus_alone_minus_both_s"] = round(med["topdown alone"] + med["render alone"] - med["both"], 4)
    print(json.dumps(row))
