#!/usr/bin/env python
"""What the identity pass costs (csrc/box_histogram.hip, identity.scan).  GPU only.

(a) ``Engine.box_histograms`` on --frames frames of 1280 x 720 resident in HBM with 4 and with 16 rectangles per frame — the torso
    rectangles (``identity.torso_rect``) of scripted boxes of 60 .. 180 x 150 .. 400 pixels — in one session: --rounds rounds of
    [warm-up calls, then --reps calls between one pair of HIP events on the engine's stream (``pa_engine_timer_start / _stop``)] per
    list, the lists taking turns.  The calls rotate over three frame sets.  The call is synchronous: its event pair includes the upload
    of the list, the read-back of k x 2 KB and the host's wait.  Reported: the median and the fastest round in microseconds per call,
    rectangles and sampled pixels per call, and GB/s of the pixels' bytes (3 per pixel).
(b) ``identity.scan`` (4 scripted boxes per frame) over a ``.y4m`` of --clip-frames such frames, in frames/s by the host clock
    (conversion on the GPU included), alternately with ``activity.scan`` (reference image given) and with one ``PlayerTracker`` run of
    ``TrackingRunner`` over the same file: --scan-rounds rounds of [activity.scan, identity.scan, tracker run].

    python tools/identity_bench.py [--frames 64] [--reps 30] [--warmup 5] [--rounds 5] [--clip-frames 128] [--scan-rounds 3] [--skip-scan]
"""
import argparse, contextlib, json, statistics, sys, tempfile, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def scripted_boxes(n, per_frame, h, w, seed=5):
    """(n, per_frame, 4) float32 xyxy: people-sized boxes inside the frame that drift a pixel or two per frame."""
    rng = np.random.default_rng(seed)
    bw, bh = rng.uniform(60, 180, per_frame), rng.uniform(150, 400, per_frame)
    x = rng.uniform(0, w - bw)[None] + np.cumsum(rng.uniform(-2, 2, (n, per_frame)), 0)
    y = rng.uniform(0, h - bh)[None] + np.cumsum(rng.uniform(-1, 1, (n, per_frame)), 0)
    x, y = np.clip(x, 0, w - bw), np.clip(y, 0, h - bh)
    return np.stack([x, y, x + bw, y + bh], -1).astype(np.float32)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--clip-frames", type=int, default=128)
    ap.add_argument("--scan-rounds", type=int, default=3)
    ap.add_argument("--skip-scan", action="store_true")
    a = ap.parse_args()
    from padel_analytics_amd import activity as A, engine as E, identity as I, render as R, video
    from padel_analytics_amd.trackers.players_tracker import Players
    from tests import synth                                     # seeded frames (setup only)
    eng = E.default_engine(0)
    n, h, w = a.frames, a.height, a.width
    fb = h * w * 3
    print("# " + " ".join(["python", "tools/identity_bench.py"] + sys.argv[1:]))
    base = synth.synthetic_frames(16, h, w, seed=1000)
    bgr = np.concatenate([np.roll(base, 7 * k, axis=2) for k in range((n + 15) // 16)])[:n]       # n distinct frames, cheaply

    # ---- (a) the kernel, two lists taking turns
    SETS = 3
    src = [eng.alloc(n * fb).upload(np.roll(bgr, k, axis=0)) for k in range(SETS)]
    lists = {}
    for per in (4, 16):
        boxes = scripted_boxes(n, per, h, w)
        rects = np.array([(i,) + I.torso_rect(boxes[i, p], h, w) for i in range(n) for p in range(per)], np.int32)
        lists[per] = rects
        got = eng.box_histograms(src[0], n, h, w, rects[:8])
        assert np.array_equal(got, I.box_histograms_host(bgr, rects[:8])), per
    out = np.zeros((n * 16, 512), np.uint32)
    times = {per: [] for per in lists}
    for _ in range(a.rounds):
        for per, rects in lists.items():
            for i in range(a.warmup):
                eng.box_histograms(src[i % SETS], n, h, w, rects, out=out)
            eng.synchronize()
            eng.timer_start()
            for i in range(a.reps):
                eng.box_histograms(src[i % SETS], n, h, w, rects, out=out)
            times[per].append(eng.timer_stop() / a.reps)
    for per, rects in lists.items():
        med, best = statistics.median(times[per]), min(times[per])
        pixels = int(((rects[:, 3] - rects[:, 1]) * (rects[:, 4] - rects[:, 2])).sum())
        print(json.dumps({"what": f"box_histograms {n} frames x {per} boxes", "us_per_call_median": round(med * 1e3, 1),
                          "us_per_call_min": round(best * 1e3, 1), "rounds": a.rounds, "reps": a.reps, "rectangles": len(rects),
                          "pixels": pixels, "median_rect_w": int(np.median(rects[:, 3] - rects[:, 1])),
                          "median_rect_h": int(np.median(rects[:, 4] - rects[:, 2])), "frames_per_s": round(n / (med * 1e-3)),
                          "GB_per_s_of_sampled_pixels": round(3 * pixels / (med * 1e-3) / 1e9, 1)}))
    for b in src[1:]:
        b.free()

    # ---- (b) the scans over a file, beside one tracker
    if not a.skip_scan:
        from padel_analytics_amd import checkpoint, detections as D, yolo_arch
        from padel_analytics_amd.trackers import PlayerTracker, TrackingRunner
        tmp = Path(tempfile.mkdtemp(prefix="identity_bench_"))
        m = a.clip_frames
        sink = video.Y4mSink(tmp / "clip.y4m", w, h, fps=30)        # the file, written by the GPU: frames 0 .. m - 1 of set 0, cyclically
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
        path = str(tmp / "clip.y4m")
        ref = np.median(base, 0).astype(np.uint8)
        boxes = scripted_boxes(m, 4, h, w)
        results = [Players(rows=np.concatenate([boxes[i], np.full((4, 1), 0.9, np.float32), np.zeros((4, 1), np.float32)], 1),
                           ids=np.arange(1, 5)) for i in range(m)]
        checkpoint.save_checkpoint(tmp / "players.pt", yolo_arch.synth_state_dict("n", 80, None, seed=3, cls_bias=0.0), "detect", 80, None, "n", {0: "person"})
        zone = D.PolygonZone(np.array([[40, 40], [w - 40, 40], [w - 40, h - 40], [40, h - 40]]), frame_resolution_wh=(w, h))
        with contextlib.redirect_stdout(sys.stderr):
            tracker = PlayerTracker(str(tmp / "players.pt"), zone, batch_size=64)
            TrackingRunner([tracker], path, tmp / "out.mp4", engine=eng).run()             # warm-up: plan, kernels
        A.scan(path, ref=ref, engine=eng)                                                  # warm-up: the file opened, the staging allocated
        tracks = I.scan(path, results, engine=eng)
        assert sorted(tracks) == [1, 2, 3, 4] and all(t.boxes == m for t in tracks.values())
        secs = {"activity": [], "identity": [], "tracker": []}
        for _ in range(a.scan_rounds):
            t0 = time.perf_counter()
            A.scan(path, ref=ref, engine=eng)
            secs["activity"].append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            I.scan(path, results, engine=eng)
            secs["identity"].append(time.perf_counter() - t0)
            with contextlib.redirect_stdout(sys.stderr):
                tracker.restart()
                runner = TrackingRunner([tracker], path, tmp / "out.mp4", engine=eng)
                runner.run()
            secs["tracker"].append(runner.timings["players_tracker"]["seconds"])
        tracker.model.close()
        med = {k: statistics.median(v) for k, v in secs.items()}
        print(json.dumps({"what": "scans of a .y4m file, 4 boxes per frame", "frames": m, "rounds": a.scan_rounds,
                          "identity_scan_ms": round(med["identity"] * 1e3, 2), "identity_scan_frames_per_s": round(m / med["identity"], 1),
                          "activity_scan_ms": round(med["activity"] * 1e3, 2), "activity_scan_frames_per_s": round(m / med["activity"], 1),
                          "players_tracker_ms": round(med["tracker"] * 1e3, 2), "players_tracker_frames_per_s": round(m / med["tracker"], 1),
                          "identity_scan_over_activity_scan": round(med["identity"] / med["activity"], 3),
                          "identity_scan_share_of_one_tracker_run": round(med["identity"] / med["tracker"], 3)}))
    src[0].free()
