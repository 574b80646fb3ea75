#!/usr/bin/env python
"""Throughput of YOLO11 beside YOLOv8 on the engine, measured in one run: yolo11m-pose (13 x 3 keypoints) @ 1280^2 through the
Pillow stretch and yolo11m detect (nc = 80) @ 640 letterboxed, batch 64 from 720p BGR frames resident in HBM, each next to the
YOLOv8m graph of the same task.  Timing: warm-up calls, then N timed synchronous calls (preprocessing, network, decode, NMS, the
device-to-host copy of the results); the median and the spread are reported.  One profiled pass per model gives per-op times: the
share of the two kernels YOLO11 adds (depthwise 3x3, PSA attention) comes from it.  Checkpoints are seeded and calibrated on two
frames of the clip (setup, untimed).  Measured once, nothing tuned.  GPU only.

    python tools/yolo11_bench.py [--batch 64] [--reps 10] [--warmup 3] [--dump-ops ops.csv] [--mode h2|bx3]
"""
import argparse, json, statistics, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", default=None, help="h2 | bx3 (default: PADEL_FP32_MODE / h2)")
    ap.add_argument("--dump-ops", default="", help="per-op CSV of the profiled passes of the two YOLO11 models")
    a = ap.parse_args()
    from PIL import Image
    from oracle import synth_weights, yolov8_ref as ref
    from padel_analytics_amd import engine as E, graph as G
    from tests import synth, yolo11_synth      # seeded synthetic clip and checkpoints (setup only)
    eng = E.default_engine(0)
    clip = synth.synthetic_frames(8, 720, 1280, seed=3)
    frames = np.ascontiguousarray(np.concatenate([clip] * ((a.batch + 7) // 8))[:a.batch])
    buf = eng.alloc(frames.nbytes).upload(frames)
    mode = a.mode or E.fp32_mode()
    calib = {"pose": ref.preprocess([np.asarray(Image.fromarray(f[..., ::-1].copy()).resize((1280, 1280)))[..., ::-1] for f in clip[:2]], 1280),
             "detect": ref.preprocess([f[..., ::-1] for f in clip[:2]], 640)}
    results, csv = [], []
    for family, task in (("yolov8", "pose"), ("yolo11", "pose"), ("yolov8", "detect"), ("yolo11", "detect")):
        nc, kpt, S, conf = (1, (13, 3), 1280, 0.25) if task == "pose" else (80, None, 640, 0.5)
        make = synth_weights.calibrated_state_dict if family == "yolov8" else yolo11_synth.calibrated_state_dict
        sd = make("m", nc, kpt, calib[task], conf, seed=11)
        m = E.Model(eng, G.build_yolo(sd, nc, kpt, dtype=E.graph_dtype(mode), family=family))
        m.set_max_batch(a.batch)
        kw = dict(imgsz=S, conf=conf, iou=0.7, classes=[0], reuse_outputs=True,
                  pre_mode=E.PRE_PIL_STRETCH if task == "pose" else E.PRE_LETTERBOX, channel_reverse=task == "pose")
        for _ in range(a.warmup):
            m.yolo_infer(buf, a.batch, 720, 1280, **kw)
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            counts = m.yolo_infer(buf, a.batch, 720, 1280, **kw)[2]
            times.append(time.perf_counter() - t0)
        overflow = m.take_overflow()
        eng.set_profiling(True)
        m.yolo_infer(buf, a.batch, 720, 1280, **kw)
        rows = m.profile_rows()
        eng.set_profiling(False)
        m.close()
        total = sum(r["ms"] for r in rows)
        ms_of = lambda kind: sum(r["ms"] for r in rows if r["kind"] == kind)
        med = statistics.median(times)
        out = {"model": f"{family}m-{task} @ {S} from 1280x720 BGR frames resident in HBM", "batch": a.batch, "arithmetic": mode, "reps": a.reps,
               "frames_per_s": round(a.batch / med, 1), "ms_per_batch_median": round(1e3 * med, 3),
               "ms_per_batch_min_max": [round(1e3 * min(times), 3), round(1e3 * max(times), 3)],
               "detections_per_frame": round(float(np.mean(counts)), 1), "h2_overflow": bool(overflow),
               "profiled_pass_ms": {"all_kernels": round(total, 3), "convs": round(ms_of(G.OP_CONV), 3),
                                    "depthwise3x3": round(ms_of(G.OP_DWCONV3), 3), "psa_attention": round(ms_of(G.OP_PSA_ATTN), 3)},
               "share_of_new_kernels": {"depthwise3x3": round(ms_of(G.OP_DWCONV3) / total, 4), "psa_attention": round(ms_of(G.OP_PSA_ATTN) / total, 4)}}
        results.append(out)
        print(json.dumps(out), flush=True)
        if family == "yolo11":
            for r in rows:
                tf = r["flops"] / r["ms"] / 1e9 if r["ms"] > 0 and r["flops"] else 0.0
                csv.append(f"{family}m-{task},{r['kind']},{r['ksize']},{r['M']},{r['cout']},{r['cin']},{r['stride']},{r['res']},{r['tile']},"
                           f"{r['family']},{r['ms']:.5f},{r['flops']:.0f},{tf:.1f}")
    if a.dump_ops:
        with open(a.dump_ops, "w") as f:
            f.write("model,kind,ksize,M,cout,cin,stride,res,tile,family,ms,flops,tflops\n" + "\n".join(csv) + "\n")
    buf.free()
