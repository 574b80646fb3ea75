#!/usr/bin/env python
"""bench.py — frames/sec of the trackers' hot path on MI355X (BASELINE.json metric), measured THROUGH the plugin
layer: `TrackingRunner.run()` (reference trackers/runner.py:175-236) drives the three real tracker classes over a
synthetic 1280x720 BGR clip that is resident in HBM; per batch of 64 frames each tracker runs preprocessing ->
network forward -> decode -> NMS on the GPU and Detections / PolygonZone / ByteTrack / result objects on the host.

One "step" = one batch of 64 frames through ALL trackers of the workload.  The timed region is ONE runner.run() over
a clip of K batches (tracker after tracker over the whole clip, exactly how the reference walks a video,
runner.py:185), bracketed by barriers; value = world x 64 x K / seconds.  `engine_only` repeats the same K steps
calling the C-ABI directly (the number round 1 reported as `value`).

One process per GPU: `python bench.py --gpus N` spawns the N ranks itself (re-exec under torch.distributed.run) unless
it is already running under a launcher (RANK in the environment).  Frames shard by batch, per-GPU batch fixed (weak
scaling); the only collective on the path is the one-time RCCL broadcast of the packed weight blobs, HBM to HBM,
inside libpadel_hip.so (pa_engine_bcast_weights) — executed at N=1 too.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload c2|c3|c4] [--batch 64] [--dump-outputs DIR] [--full]

A plain run does what the headline needs and nothing else: set-up, W warm-up steps, the K timed steps, the outputs of
`--dump-outputs`, and ONE JSON line (rank 0) with the driver's contract fields.  `--full` adds every other leg to that
line: `engine_only` (and the strict-fp32 kernels beside it), `objects_materialised`, `value_lazy_objects`,
`value_eager_objects`, `host_frames`, `reference_default`, `roofline` (per-op profile, PMC traffic passes), `cpu_baseline`
and `parity` (`parity.low_noise_heads`: the same graphs with well-conditioned heads, where the literal 1e-3 px bar is
checked), at N > 1 `replica_runners`; the `--no-*` options and `--quick` drop legs of a `--full` run.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

PEAK_FP32_MFMA_TFLOPS = 157.3      # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32, dense
PEAK_FP16_MFMA_TFLOPS = 2500.0     # same guide: BF16/FP16 MFMA, dense (not the 2:1-sparsity headline)
# default fp32 path = bf16x3 kernels: every fp32 multiply costs 6 bf16 products on the bf16 pipe
PEAK_BX3_TFLOPS = round(PEAK_FP16_MFMA_TFLOPS / 6.0, 1)
# h2 path (default since round 3): activations as fp16 pairs, every fp32 multiply costs 3 f16 products on the same pipe
PEAK_H2_TFLOPS = round(PEAK_FP16_MFMA_TFLOPS / 3.0, 1)
SUSTAINED_FP16_MFMA_TFLOPS = 1780.0     # measured on random operands, 16x16x32 AND 32x32x16 f16 (profiles/r4a_mfma_f16_ubench.txt: 1.71-1.85 PFLOP/s;
                                        # all-zero operands reach 2.2-2.5): reported beside the nominal peak, never instead of it
PEAK_BY_IMPL = {"h2": PEAK_H2_TFLOPS, "bx3": PEAK_BX3_TFLOPS, "tap": PEAK_FP32_MFMA_TFLOPS}

# tracker table: name -> (scale, nc, kpt_shape, imgsz, conf, classes, pre_mode, channel_reverse)
TRACKERS = {
    # reference default players model is yolov8m.pt (config.py:22), COCO-80, classes=[0], conf .5
    "players": dict(scale="m", nc=80, kpt=None, imgsz=640, conf=0.5, classes=[0], pre="letterbox", rev=False),
    # BASELINE configs name a YOLOv8 detect instance for the ball (nc=1); no reference scale -> n
    "ball": dict(scale="n", nc=1, kpt=None, imgsz=640, conf=0.25, classes=None, pre="letterbox", rev=False),
    # 13-keypoint pose at train_image_size 1280 (config.py:29-31), conf .25; custom checkpoint of unknown
    # scale in the reference -> same family as the players default (m)
    "pose": dict(scale="m", nc=1, kpt=(13, 3), imgsz=1280, conf=0.25, classes=[0], pre="pil", rev=True),
}
WORKLOADS = {
    "c2": ("BASELINE configs[1]: 1280x720 batch=64, players + ball YOLOv8 detect", ["players", "ball"]),
    "c3": ("BASELINE configs[2]: 1280x720 batch=64, players + ball detect + 13-kpt pose", ["players", "ball", "pose"]),
    # configs[4] is 8 x 64 frames of 1920x1080 in fp16: one GPU's shard of it (forces --height 1080 --width 1920 --dtype f16)
    "c4": ("BASELINE configs[4], one GPU's shard: 1920x1080 fp16 batch=64 (512 over 8 GPUs), all trackers + batched NMS",
           ["players", "ball", "pose"]),
}
# court-like zone for the players tracker (main.py:108-119 builds it from court corners k1, k2, k12, k11)
ZONE_720P = [[260, 170], [1020, 170], [1240, 700], [40, 700]]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="c3", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=64, help="frames per GPU per step")
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--scales", default="", help="override scales, e.g. players=n,pose=n")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beside the headline: engine-only, lazy / eager result objects, host frames, the reference's "
                         "default trackers, roofline, CPU baseline and parity (minutes; a plain run times the headline alone)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the CPU oracle leg (cpu_baseline and parity)")
    ap.add_argument("--no-fp64", action="store_true", help="parity leg: skip the fp64 oracle (noise floor)")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--engine-only", action="store_true", help="skip the runner-level measurement (profiling runs)")
    ap.add_argument("--no-compare", action="store_true", help="skip the fp32-MFMA comparison leg of engine_only (profiling runs)")
    ap.add_argument("--cpu-sample", type=int, default=0, help="frames of the CPU baseline sample (0 = auto)")
    ap.add_argument("--dump-ops", default="", help="write the per-op profile (CSV) of the roofline pass here")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the timed path returned for its last step as DIR/<tracker>.npy (float64, rank 0; "
                         "at most 64 MB in all: larger outputs are cut to a seeded sample of rows)")
    ap.add_argument("--no-host-frames", action="store_true",
                    help="skip the end-to-end-from-host leg (clip in page-locked host memory: sequential = one upload per "
                         "tracker like the reference, fan-out = one upload per batch — PCIe-inclusive rates)")
    ap.add_argument("--no-reference-default", action="store_true",
                    help="skip the leg with the reference's own default configuration (players yolov8m + pose + the "
                         "TrackNetV3 BallTracker, config.py:22,29-30,36-39)")
    ap.add_argument("--graph", type=int, default=-1, help="hipGraph replay of the op lists (tuning; -1 = engine default)")
    ap.add_argument("--impl", default="h2", choices=["h2", "bx3", "tap"],
                    help="fp32-equivalent conv arithmetic: h2 (default: activations as fp16 pairs, 3 products on the f16 matrix "
                         "pipe, corrections in their own accumulator), bx3 (exact 3-way bf16 split, 6 products; the full-range "
                         "fallback of h2), tap (fp32-input MFMA: the strict-fp32 kernels)")
    ap.add_argument("--replay", type=int, default=0, help="tuning: frames per pass over the op list (0 = the whole batch)")
    ap.add_argument("--fake-engine", action="store_true",
                    help="TEST ONLY (tests/test_bench_gloo.py): run main() over tests/fake_engine.py with the gloo backend — the "
                         "launcher contract, barriers, max-over-ranks timing and the weight broadcast without a GPU; the line "
                         "carries \"fake_engine\": true and is not a measurement")
    ap.add_argument("--traffic", default="live", choices=["live", "static", "none"],
                    help="roofline.traffic: live = two rocprofv3 --pmc passes over this script's engine-only step (needs rocprofv3; "
                         "falls back to static), static = the committed measurement profiles/r6_traffic.json")
    ap.add_argument("--no-eager", action="store_true", help="skip the eager-result-objects leg (value_eager_objects)")
    ap.add_argument("--quick", action="store_true", help="tuning runs: runner + engine-only + roofline only (no CPU leg, host-frames leg, reference-default leg)")
    ap.add_argument("--no-tight", action="store_true", help="skip the low-noise-head parity leg of the CPU baseline section")
    ap.add_argument("--dtype", default="f32", choices=["f32", "f16"],
                    help="f32: the parity path (the reference runs half=False) — the headline; f16: fp16 activations / "
                         "weights with fp32 accumulation (BASELINE configs[4]), reports its own L-inf vs the fp32 oracle")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps: at least one timed step")
    if a.dump_ops and not a.full:
        ap.error("--dump-ops: the per-op profile belongs to the roofline leg, which runs with --full")
    if not a.full:
        a.quick = a.no_roofline = True
    if a.fake_engine:
        a.quick = a.no_roofline = True
    if a.quick:
        a.no_cpu_baseline = a.no_host_frames = a.no_reference_default = a.no_eager = a.no_compare = True
        if a.traffic == "live":
            a.traffic = "static"
    return a


def source_for_oracle(cfg, frames):
    """What the reference hands to YOLO.predict for these frames (players_tracker.py:346-349,
    players_keypoints_tracker.py:260-266) — used for weight calibration and the CPU baseline."""
    if cfg["pre"] == "pil":
        from PIL import Image
        S = cfg["imgsz"]
        return [np.asarray(Image.fromarray(f[..., ::-1].copy()).resize((S, S)))[..., ::-1] for f in frames]
    return [f[..., ::-1] for f in frames]


_SD_CACHE = {}


def _pmc_summary():
    """MfmaUtil of the dominant kernel from the committed PMC pass of this round (static: a counter pass cannot run inside the bench)."""
    p = ROOT / "profiles" / "r6_pmc_summary.json"
    try:
        return json.loads(p.read_text())
    except Exception:
        return {}


PMC_SUMMARY = _pmc_summary()
HBM_PEAK_TBS, HBM_ACHIEVABLE_TBS = 8.0, 6.3           # MI355X_MICROARCH.md: spec / measured float4 copy


def conv1x1_roofline(c1, fl1, ms1, peak1, a):
    """1x1 convs priced twice: against the matrix pipe, and — the big-M, small-K ones are HBM-bound on the 4-byte-per-
    channel pair storage — against HBM: algorithmic bytes = M x (cin + cout) x 4 (activations in and out once; weights are L2-resident).
    Per layer the bound is whichever roof gives the longer time; `hbm_bound` / `mfma_bound` sum the layers of each class."""
    es = 2 if a.dtype == "f16" else 4
    cls = {"hbm": [0.0, 0.0, 0.0, 0], "mfma": [0.0, 0.0, 0.0, 0]}      # ms, bytes, flops, launches
    for r in c1:
        byts = float(r["M"]) * (r["cin"] + r["cout"] * (1 + int(r.get("res", 0)))) * es
        t_hbm = byts / (HBM_ACHIEVABLE_TBS * 1e12)
        t_mfma = r["flops"] / (peak1 * 1e12)
        k = "hbm" if t_hbm >= t_mfma else "mfma"
        cls[k][0] += r["ms"]; cls[k][1] += byts; cls[k][2] += r["flops"]; cls[k][3] += 1
    out = {"achieved": round(fl1 / (ms1 * 1e-3) / 1e12, 2) if ms1 > 0 else 0.0, "ms_per_step": round(ms1, 3),
           "peak": peak1, "frac": round(fl1 / (ms1 * 1e-3) / 1e12 / peak1, 4) if ms1 > 0 else 0.0}
    h, m = cls["hbm"], cls["mfma"]
    out["hbm_bound"] = {"bound": "hbm", "launches": h[3], "ms_per_step": round(h[0], 3),
                        "tb_per_s": round(h[1] / (h[0] * 1e-3) / 1e12, 3) if h[0] > 0 else 0.0, "peak_tb_per_s": HBM_PEAK_TBS,
                        "frac": round(h[1] / (h[0] * 1e-3) / 1e12 / HBM_PEAK_TBS, 4) if h[0] > 0 else 0.0,
                        "frac_of_achievable_6p3": round(h[1] / (h[0] * 1e-3) / 1e12 / HBM_ACHIEVABLE_TBS, 4) if h[0] > 0 else 0.0}
    out["mfma_bound"] = {"bound": "mfma", "launches": m[3], "ms_per_step": round(m[0], 3),
                         "tflop_per_s": round(m[2] / (m[0] * 1e-3) / 1e12, 2) if m[0] > 0 else 0.0, "peak": peak1,
                         "frac": round(m[2] / (m[0] * 1e-3) / 1e12 / peak1, 4) if m[0] > 0 else 0.0}
    return out


def make_state_dict(name, cfg, frames, frac=0.01, seed_offset=0, calib_dtype="f32"):
    """Setup (untimed): seeded synthetic checkpoint with data-calibrated BatchNorm statistics
    (oracle/synth_weights.py — weight synthesis, not part of the measured path).  1280-input models
    are calibrated on a 640x640 centre crop of the network input (same statistics, 4x cheaper).
    ``calib_dtype="f64"``: the calibration pass in double precision, which makes the checkpoint independent of torch's thread count
    (synth_weights.calibrated_state_dict).  The benchmark's own checkpoints are and stay made with the fp32 pass, so their weights
    follow the host's thread count too: figures of two hosts are figures on slightly different weights."""
    import zlib
    # (the fingerprint of the calibration frames is part of the key: tests build the same tracker for different clips)
    key = (name, cfg["scale"], cfg["nc"], cfg["kpt"], cfg["imgsz"], frac, seed_offset, zlib.crc32(np.ascontiguousarray(frames[:2]).tobytes())) + \
        ((calib_dtype,) if calib_dtype != "f32" else ())
    if key in _SD_CACHE:
        return _SD_CACHE[key]
    # the PMC passes of the roofline section re-run this script under rocprofv3: they find the checkpoints of the parent here
    cdir = os.environ.get("PADEL_BENCH_SD_CACHE")
    cfile = Path(cdir) / ("sd_" + "_".join(str(k) for k in key).replace(" ", "").replace("(", "").replace(")", "").replace(",", "x") + ".npz") if cdir else None
    if cfile is not None and cfile.exists():
        with np.load(cfile) as z:
            sd = {k: z[k] for k in z.files}
        _SD_CACHE[key] = sd
        return sd
    import torch
    from oracle import synth_weights, yolov8_ref as ref
    srcs = source_for_oracle(cfg, frames[:2])
    im = ref.preprocess(srcs, cfg["imgsz"])
    if im.shape[2] > 640:
        o = (im.shape[2] - 640) // 2
        im = im[:, :, o:o + 640, o:o + 640].contiguous()
    sd = synth_weights.calibrated_state_dict(cfg["scale"], cfg["nc"], cfg["kpt"], im, cfg["conf"],
                                             seed=sum(map(ord, name)) + seed_offset, frac=frac,
                                             dtype={"f32": torch.float32, "f64": torch.float64}[calib_dtype])
    _SD_CACHE[key] = sd
    if cfile is not None:
        np.savez(cfile, **{k: np.asarray(v) for k, v in sd.items()})
    return sd


# every kernel a 3x3 conv op of the graph can be launched as (conv_tap_h2.hip:launch_conv_h2's dispatch)
H2_CONV3_KERNELS = {"h2": ("conv_h2p_kernel", "conv_h2q_kernel", "conv_h2w_kernel", "conv_h2_kernel", "conv_h2r_kernel", "conv_h2v_kernel",
                           "conv_h2s3_kernel"),
                    "bx3": ("conv_bx3p_kernel", "conv_bx3_kernel"), "tap": ("conv_tap_kernel",)}


def measure_traffic(a, ops_rows, tmp):
    """HBM bytes of the dominant kernels (every 3x3 conv launch of one step), per launch, from the PMC counters collected
    exactly as /opt/skills/guides/MI355X_MICROARCH.md prescribes: FETCH_SIZE and WRITE_SIZE in SEPARATE rocprofv3 --pmc
    passes with --kernel-trace only, over this script's own engine-only step; FETCH_SIZE (KiB) x 1024 x 2 (gfx950 tallies
    the 128-byte requests of wide coalesced reads, `buffer_load ... lds` included, at 64 B), WRITE_SIZE (KiB) x 1024 as is.
    Returns None when rocprofv3 is not there or a pass fails (the caller falls back to the committed measurement)."""
    import csv
    import glob
    import shutil
    if shutil.which("rocprofv3") is None:
        return None
    kernels = H2_CONV3_KERNELS[a.impl]
    tot = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        d = Path(tmp) / f"pmc_{counter}"
        cmd = ["rocprofv3", "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", str(d), "-o", "p", "--",
               sys.executable, str(Path(__file__).resolve()), "--workload", a.workload, "--impl", a.impl, "--steps", "1", "--warmup", "1",
               "--batch", str(a.batch), "--height", str(a.height), "--width", str(a.width), "--quick", "--engine-only", "--no-roofline"]
        if a.scales:
            cmd += ["--scales", a.scales]
        env = dict(os.environ, TMPDIR="/tmp", PADEL_BENCH_SD_CACHE=str(tmp))
        try:
            r = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
        except (subprocess.TimeoutExpired, OSError):
            return None
        if r.returncode != 0:
            sys.stderr.write(f"bench: PMC pass {counter} failed (rc {r.returncode}): {r.stderr.decode(errors='replace')[-400:]}\n")
            return None
        v, disp = 0.0, set()
        for f in glob.glob(f"{d}/**/*counter_collection.csv", recursive=True):
            for row in csv.DictReader(open(f)):
                if row["Counter_Name"] == counter and any(k + "<" in row["Kernel_Name"] for k in kernels):
                    v += float(row["Counter_Value"])
                    disp.add((f, row["Dispatch_Id"]))
        if not disp:
            return None
        tot[counter] = (v, len(disp))
        shutil.rmtree(d, ignore_errors=True)
    alg, n_ops = 0.0, 0
    for r in ops_rows:
        if r["kind"] == 2 and r["ksize"] == 3:
            st = r["stride"]
            alg += r["M"] * st * st * r["cin"] * 4 + r["M"] * r["cout"] * 4 + 9 * r["cin"] * r["cout"] * (6 if a.impl == "bx3" else 4)
            alg += r["M"] * r["cout"] * 4 * int(r.get("res", 0))          # a conv that adds a residual input reads it
            n_ops += 1
    if not n_ops:
        return None
    # the counted launches must be whole steps of exactly the graph's 3x3 ops: an average over a subset (a kernel name missing from
    # the list above) would be compared with the wrong algorithmic figure
    for c in ("FETCH_SIZE", "WRITE_SIZE"):
        if tot[c][1] % n_ops:
            sys.stderr.write(f"bench: PMC pass {c} counted {tot[c][1]} launches of the 3x3 kernels, the graph has {n_ops} per step: not used\n")
            return None
    fetch = tot["FETCH_SIZE"][0] * 1024 * 2 / tot["FETCH_SIZE"][1]
    write = tot["WRITE_SIZE"][0] * 1024 / tot["WRITE_SIZE"][1]
    return {"bytes_per_launch": round(fetch + write), "fetch_bytes_per_launch": round(fetch), "write_bytes_per_launch": round(write),
            "algorithmic_bytes_per_launch": round(alg / n_ops), "ratio_to_algorithmic": round((fetch + write) / (alg / n_ops), 3),
            "launches_counted": {"FETCH_SIZE": tot["FETCH_SIZE"][1], "WRITE_SIZE": tot["WRITE_SIZE"][1], "ops_per_step": n_ops},
            "static": False,
            "source": "this run: rocprofv3 --pmc FETCH_SIZE | WRITE_SIZE (separate passes) of one engine-only step; FETCH x 2 (gfx950)"}


def parity_low_noise_heads(eng, names, frames, sample, H, W, ref, parity):
    """The literal north_star bar.  The same graphs, frames and weights as the timed run except for the LAST conv of the
    DFL (and keypoint) branch of each head, scaled down until the fp32 CPU oracle itself is reproducible to the ulp of
    the pixel coordinates: there `engine vs reference CPU path <= 1e-3 px` is a meaningful statement, and it is checked
    (tests/test_gpu_yolo_parity.py::test_*_tight assert the same on the GPU box)."""
    import torch
    from padel_analytics_amd import engine as E, graph as G
    ns = len(sample)
    res = {"linf_px_vs_fp32_oracle": 0.0, "linf_px_vs_fp64": 0.0, "oracle_floor_px": 0.0, "detections": 0, "per_tracker": {},
           "within_1e-3_px": True,
           "what": "last conv of model.22.cv2 (DFL) and cv4 (keypoints) scaled by f; everything else as timed"}
    for name in names:
        cfg = TRACKERS[name]
        f = 0.004 if cfg["imgsz"] > 640 else 0.02
        sd = dict(make_state_dict(name, cfg, frames))
        for branch in ("cv2", "cv4"):
            for l in range(3):
                for nm in ("weight", "bias"):
                    k = f"model.22.{branch}.{l}.2.{nm}"
                    if k in sd:
                        sd[k] = (sd[k] * np.float32(f)).astype(np.float16).astype(np.float32)
        srcs = source_for_oracle(cfg, sample)
        r32 = ref.predict(ref.YoloV8Ref(sd, cfg["nc"], cfg["kpt"]), srcs, cfg["conf"], 0.7, cfg["imgsz"], cfg["classes"])
        r64 = ref.predict(ref.YoloV8Ref(sd, cfg["nc"], cfg["kpt"], dtype=torch.float64), srcs, cfg["conf"], 0.7,
                          cfg["imgsz"], cfg["classes"])
        m = E.Model(eng, G.build_yolov8(sd, cfg["nc"], cfg["kpt"], dtype=E.graph_dtype()))
        m.set_max_batch(ns)
        boxes, kpts, counts = m.yolo_infer(np.ascontiguousarray(sample), ns, H, W, imgsz=cfg["imgsz"], conf=cfg["conf"], iou=0.7,
                                           classes=cfg["classes"],
                                           pre_mode=E.PRE_PIL_STRETCH if cfg["pre"] == "pil" else E.PRE_LETTERBOX,
                                           channel_reverse=cfg["rev"])
        m.close()
        nk = 0 if cfg["kpt"] is None else cfg["kpt"][0] * cfg["kpt"][1]
        b64 = np.zeros((ns, 300, 6), np.float32)
        k64 = np.zeros((ns, 300, nk), np.float32) if nk else None
        c64 = np.zeros(ns, np.int32)
        for i, r in enumerate(r64):
            c64[i] = len(r["boxes"])
            b64[i, :c64[i]] = r["boxes"]
            if nk and c64[i]:
                k64[i, :c64[i]] = r["kpts"].reshape(c64[i], -1)
        entry = {"f": f}
        try:
            floor = parity.compare_batch(r32, b64, k64, c64, cfg["conf"], 0.7, kpt_shape=cfg["kpt"])
            g32 = parity.compare_batch(r32, boxes, kpts, counts, cfg["conf"], 0.7, kpt_shape=cfg["kpt"])
            g64 = parity.compare_batch(r64, boxes, kpts, counts, cfg["conf"], 0.7, kpt_shape=cfg["kpt"])
            entry.update(detections=g32["n"], linf_px_vs_fp32_oracle=round(g32["worst_px"], 6),
                         linf_px_vs_fp64=round(g64["worst_px"], 6), oracle_floor_px=round(floor["worst_px"], 6))
            res["detections"] += g32["n"]
            for k, v in (("linf_px_vs_fp32_oracle", g32["worst_px"]), ("linf_px_vs_fp64", g64["worst_px"]),
                         ("oracle_floor_px", floor["worst_px"])):
                res[k] = round(max(res[k], v), 6)
        except AssertionError as e:
            entry["mismatch"] = str(e)[:300]
            res["within_1e-3_px"] = False
        res["per_tracker"][name] = entry
    res["within_1e-3_px"] = bool(res["within_1e-3_px"] and res["detections"] > 0 and
                                 max(res["linf_px_vs_fp32_oracle"], res["linf_px_vs_fp64"]) <= 1e-3)
    return res


def spawn_ranks(a) -> int:
    """`python bench.py --gpus N` outside a launcher: become `python -m torch.distributed.run ... bench.py ...`."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(Path(__file__).resolve())] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)


def build_trackers(names, frames, rank, B, H, W, eng, tmp, half=False, frac=0.01, tag="", replay=0, sd_override=None):
    """The three plugin classes exactly as main.py:126-161 constructs them, over synthetic checkpoints.  Only rank 0
    synthesises / "loads" real weights; the other ranks create their models from an architecture-only checkpoint
    with an EMPTY weight blob in HBM and receive rank 0's blob through pa_engine_bcast_weights."""
    from padel_analytics_amd import checkpoint, detections as D, yolo_arch
    from padel_analytics_amd.trackers import BallDetectTracker, PlayerKeypointsTracker, PlayerTracker
    trackers, flops = {}, {}
    for name in names:
        cfg = TRACKERS[name]
        sd = (sd_override[name] if sd_override else make_state_dict(name, cfg, frames, frac[name] if isinstance(frac, dict) else frac)) \
            if rank == 0 else yolo_arch.synth_state_dict(cfg["scale"], cfg["nc"], cfg["kpt"], 0)
        path = Path(tmp) / f"{name}{tag}_r{rank}.pt"
        checkpoint.save_checkpoint(path, sd, "pose" if cfg["kpt"] else "detect", cfg["nc"], cfg["kpt"], cfg["scale"],
                                   {0: "person" if name != "ball" else "ball"})
        if name == "players":
            sx, sy = W / 1280.0, H / 720.0
            zone = D.PolygonZone(np.array([[int(x * sx), int(y * sy)] for x, y in ZONE_720P]), frame_resolution_wh=(W, H))
            t = PlayerTracker(str(path), zone, batch_size=B, half=half)
        elif name == "pose":
            t = PlayerKeypointsTracker(str(path), cfg["imgsz"], batch_size=B, half=half)
        else:
            t = BallDetectTracker(str(path), batch_size=B, conf=cfg["conf"], half=half)
        # frames per graph replay: the whole batch (measured on c3 in round 1: 16 -> 247, 32 -> 256, 64 -> 264
        # frames/s; small replays leave the P5 layers with ~2 rounds of workgroups)
        t.model.set_max_batch(replay or B)
        t.model.attach(eng, receive_weights=rank != 0)
        t.model.broadcast_weights(root=0)                 # RCCL, HBM -> HBM (a self-broadcast at N=1)
        trackers[name] = t
        S = cfg["imgsz"]
        if cfg["pre"] == "pil":
            nh = nw = S
        else:
            r = min(S / H, S / W)
            nw, nh = int(round(W * r)), int(round(H * r))
            nw, nh = nw + (S - nw) % 32, nh + (S - nh) % 32
        flops[name] = yolo_arch.conv_flops(yolo_arch.conv_inventory(cfg["scale"], cfg["nc"], cfg["kpt"], nh, nw))
    return trackers, flops


# --dump-outputs: under 64 MB in all, .npy headers included, whether MB means 10^6 or 2^20 bytes
DUMP_LIMIT_BYTES = 60 << 20


def runner_outputs(trackers, frames_idx):
    """What TrackingRunner.run() left its caller for the frames `frames_idx`, one float64 table per tracker with the frame
    index in column 0: players = x1, y1, x2, y2, confidence, class id, track id (-1: none) per player; pose = x, y (source
    pixels) of every keypoint per person; ball = x, y, visibility per frame."""
    out = {}
    for name, t in trackers.items():
        preds, rows = t.results.predictions, []
        for f in frames_idx:
            if name == "players":
                rows += [[f, *p.xyxy, p.confidence, p.class_id, -1 if p.id is None else p.id] for p in preds[f].players]
            elif name == "pose":
                rows += [[f, *(v for k in person.player_keypoints for v in k.xy)] for person in preds[f].players_keypoints]
            else:
                rows.append([f, *preds[f].xy, preds[f].visibility])
        width = {"players": 8, "ball": 4}.get(name) or 1 + 2 * TRACKERS[name]["kpt"][0]
        out[name] = np.asarray(rows, np.float64).reshape(-1, width)
    return out


def engine_outputs(last):
    """What pa_yolo_infer returned in the last engine-only step, one float64 table per tracker with one row per detection:
    frame, x1, y1, x2, y2, confidence, class id, then x, y, confidence of every keypoint on pose models."""
    out = {}
    for name, (boxes, kpts, counts) in last.items():
        out[name] = np.concatenate([np.concatenate([np.full((c, 1), i), boxes[i, :c]] + ([] if kpts is None else [kpts[i, :c]]), 1)
                                    for i, c in enumerate(counts.tolist())]).astype(np.float64)
    return out


def write_outputs(d, tables):
    """DIR/<name>.npy.  Beyond DUMP_LIMIT_BYTES in all, every table keeps the same fraction of its rows, a sample drawn with
    a fixed seed (the frame column says where each kept row came from)."""
    keep = min(1.0, DUMP_LIMIT_BYTES / max(sum(x.nbytes for x in tables.values()), 1))
    Path(d).mkdir(parents=True, exist_ok=True)
    for name, x in tables.items():
        if keep < 1.0:
            x = x[np.sort(np.random.default_rng(0).choice(len(x), int(len(x) * keep), replace=False))]
        np.save(Path(d) / f"{name}.npy", x)


def main():
    a = parse()
    if a.gpus > 1 and "RANK" not in os.environ:
        sys.exit(spawn_ranks(a))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # stdout carries exactly ONE line (the JSON): everything else that writes to fd 1 — the trackers' prints, but also
    # librccl's C-level start-up banner — is pointed at stderr for the life of the process
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    import torch
    from padel_analytics_amd import dist as D, engine as E, video
    from tests import synth
    from padel_analytics_amd.trackers import TrackingRunner
    fake = None
    if a.fake_engine:
        from tests import fake_engine as fake
        fake.install()

    dist = None
    if world > 1:
        import torch.distributed as dist
        if fake is None:
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))     # barriers of the contract
        else:
            dist.init_process_group("gloo")
        # setup (weight synthesis / packing) is host work in every rank: share the cores instead of oversubscribing
        torch.set_num_threads(max(1, min(64, (os.cpu_count() or 8) // world)))

    for kv in filter(None, a.scales.split(",")):
        k, v = kv.split("=")
        TRACKERS[k]["scale"] = v
    desc, names = WORKLOADS[a.workload]
    if a.workload == "c4":
        a.height, a.width, a.dtype = 1080, 1920, "f16"
    H, W, B, K, Wm = a.height, a.width, a.batch, a.steps, a.warmup

    os.environ["PADEL_FP32_MODE"] = "h2" if a.impl == "h2" else "bx3"      # what the tracker classes build their graphs for
    eng = E.Engine(local)
    if a.graph >= 0:
        eng.set_tuning(graph=a.graph)
    IMPL = {"tap": 0, "bx3": 2, "h2": 2}
    eng.set_tuning(impl=IMPL[a.impl])
    # RCCL communicator owned by the library (also with one rank: the broadcast path is exercised at N=1)
    eng.comm_init(D.share_unique_id(E.comm_unique_id), world, rank)
    frames = synth.synthetic_frames(B, H, W, seed=1000 + rank)          # each rank its own shard
    clip = video.DeviceClip(eng, frames, repeat=max(K, Wm, 1))           # resident in HBM before timing
    tmp = tempfile.mkdtemp(prefix="padel_bench_")
    # (only a run that will start them: a plain run writes no checkpoint files)
    if a.traffic == "live" and not a.no_roofline:
        os.environ.setdefault("PADEL_BENCH_SD_CACHE", tmp)      # calibrated checkpoints on disk: the PMC sub-runs (measure_traffic) reuse them
    with contextlib.redirect_stdout(sys.stderr):
        trackers, flops_per_frame = build_trackers(names, frames, rank, B, H, W, eng, tmp, half=a.dtype == "f16", replay=a.replay)

    def fence():
        eng.synchronize()
        if world > 1:
            if fake is None:
                torch.cuda.synchronize()
            dist.barrier()
            if fake is None:
                torch.cuda.synchronize()

    def run_runner(source, n_batches, trk=None, **kw):
        """One TrackingRunner.run() over n_batches x B frames; returns seconds (max over ranks)."""
        runner = TrackingRunner(list((trk or trackers).values()), source, Path(tmp) / "out.mp4", start=0, end=n_batches * B, **kw)
        runner.restart()
        fence()
        t0 = time.perf_counter()
        runner.run()
        fence()
        dt = time.perf_counter() - t0
        return eng.allreduce_max(dt), runner

    last_infer = {}          # the arrays of the latest engine_step (--dump-outputs --engine-only)

    def engine_step():
        tot = 0
        for name in names:
            cfg = TRACKERS[name]
            boxes, kpts, counts = trackers[name].model._ensure_model().yolo_infer(
                clip.buffer, B, H, W, imgsz=cfg["imgsz"], conf=cfg["conf"], iou=0.7, classes=cfg["classes"],
                max_det=1 if name == "ball" else 300,
                pre_mode=E.PRE_PIL_STRETCH if cfg["pre"] == "pil" else E.PRE_LETTERBOX, channel_reverse=cfg["rev"],
                reuse_outputs=True)
            last_infer[name] = (boxes, kpts, counts)
            tot += int(counts.sum())
        return tot

    def fp32_mfma_leg():
        """The same engine-only steps on the STRICT fp32 kernels (fp32 storage, v_mfma_f32_16x16x4_f32: fp32 in, fp32
        accumulate, 157.3 TFLOP/s pipe) — the number that carries no equivalence argument.  h2 trackers are rebuilt on fp32
        storage for it (so it runs last on that path)."""
        for t_ in trackers.values():
            t_.model.set_fp32_mode("bx3")                  # fp32 storage graphs (what the fp32-input kernels read)
            t_.model.set_max_batch(B)
        eng.set_tuning(impl=0)
        engine_step()
        fence()
        t0_ = time.perf_counter()
        for _ in range(K):
            engine_step()
        fence()
        dt_m = eng.allreduce_max(time.perf_counter() - t0_)
        eng.set_tuning(impl=IMPL[a.impl])
        return {"value": round(world * B * K / dt_m, 2), "unit": "frames/s", "ms_per_step": round(1e3 * dt_m / K, 3),
                "what": "fp32 storage + fp32-input MFMA (v_mfma_f32_16x16x4_f32), engine-only; peak 157.3 TFLOP/s"}

    out = {
        "metric": "frames/sec (all trackers) on 1280x720", "value": None, "unit": "frames/s",
        "n_gpus": world, "steps": K, "warmup": Wm, "ms_per_step": None,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        # what the path computes in: NOT plain fp32 arithmetic on the default path — fp32-equivalent pairs of fp16
        # (every string the driver keeps is <= 120 characters: its record cuts longer ones; the prose lives in DESIGN.md §3.1 / §3.5 / §5)
        "dtype": ("f16" if a.dtype == "f16" else
                  "f32-equivalent (h2: fp16 pairs h + m/2048, 2 or 3 f16 MFMA products per multiply, fp32 accumulate)" if a.impl == "h2" else
                  "f32 (bx3: exact 3-way bf16 split, 6 bf16 MFMA products per multiply, fp32 accumulate)" if a.impl == "bx3" else
                  "f32 (fp32-input MFMA)"),
        "data": "synthetic",
        "arithmetic": ("h2: activations fp16 pairs (22-23 bits), 3 MFMA products, 2 where weights are fp16 numbers; DESIGN.md 3.1/3.5" if (a.dtype == "f32" and a.impl == "h2") else
                       "bx3: exact 3-way bf16 split of fp32 operands, 6 of 9 cross products, fp32 accumulate; DESIGN.md 3.1" if (a.dtype == "f32" and a.impl == "bx3") else
                       "fp32 storage, v_mfma_f32_16x16x4_f32" if a.dtype == "f32" else "fp16 storage, v_mfma_f32_16x16x32_f16, fp32 accumulate, fp32 heads"),
        "config": {
            "workload": desc, "frames_per_gpu_per_step": B, "frame_hw": [H, W],
            "trackers": {n: {"graph": f"yolov8{TRACKERS[n]['scale']}-{'pose13x3' if TRACKERS[n]['kpt'] else 'detect'}"
                                      f"-nc{TRACKERS[n]['nc']}", "imgsz": TRACKERS[n]["imgsz"],
                             "conv_gflop_per_frame": round(flops_per_frame[n] / 1e9, 2)} for n in names},
            "parallelism": f"frames sharded by batch over {world} GPU(s), one-time RCCL weight broadcast inside libpadel_hip.so",
            "inputs": "uint8 BGR clip resident in HBM; result objects (Players / Ball / PlayersKeypoints) on the host",
            # scalars a reader of the driver's record must not lose (filled in below)
            "engine_only_frames_per_s": None, "fp32_strict_frames_per_s": None,
            "parity_linf_px_vs_fp32_oracle": None, "parity_oracle_floor_px": None, "parity_linf_px_vs_fp64": None,
            "parity_low_noise_linf_px": None,
            "timed_path": "TrackingRunner.run(): trackers in sequence, submit k+1 before wait k; queued host stages drain beside the next tracker",
        },
    }

    with contextlib.redirect_stdout(sys.stderr):
        # ---- engine-only: K steps straight through the C-ABI (round 1's `value`)
        # (a leg of --full; with --engine-only these ARE the timed steps)
        if a.full or a.engine_only:
            ndet = 0
            for _ in range(max(Wm, 1)):
                ndet = engine_step()
            fence()
            t0 = time.perf_counter()
            for _ in range(K):
                engine_step()
            fence()
            dt_e = eng.allreduce_max(time.perf_counter() - t0)
            out["engine_only"] = {"value": round(world * B * K / dt_e, 2), "unit": "frames/s", "ms_per_step": round(1e3 * dt_e / K, 3),
                                  "what": "the same K steps calling pa_yolo_infer directly: no Detections / PolygonZone / ByteTrack / objects"}
            if a.dump_outputs and a.engine_only and rank == 0:
                write_outputs(a.dump_outputs, engine_outputs(last_infer))
            if a.dtype == "f32" and a.impl == "bx3" and not a.no_compare:
                out["engine_only"]["fp32_mfma_kernels"] = fp32_mfma_leg()
            out["config"]["detections_per_step_rank0"] = ndet
            out["config"]["engine_only_frames_per_s"] = out["engine_only"]["value"]
        elif Wm == 0:
            # --warmup 0 has never meant a cold first timed step: one untimed pass through every model (arena, captured op lists,
            # page-locked result sets) precedes the runner, as the engine-only leg did when it ran in every run
            engine_step()
        # ---- through the runner (the metric's path).  Round 5: `value` is the run with the result objects built where the
        # reference builds them — every Player / PlayerKeypoints object inside predict_sample (players_tracker.py:371-378,
        # players_keypoints_tracker.py:303-320; trackers.set_eager_objects(True): array-backed objects, ~0.5 us each); the run
        # that leaves them to first access is the side number `value_lazy_objects`
        from padel_analytics_amd import trackers as T
        if not a.engine_only:
            T.set_eager_objects(True)
            if world == 1 or a.full:          # at N > 1 the replica runners are a leg of --full: `value` is the sharded runner below
                if Wm > 0:
                    run_runner(clip, Wm)
                dt, runner = run_runner(clip, K)
                out["value"] = round(world * B * K / dt, 2)
                out["ms_per_step"] = round(1e3 * dt / K, 3)
                out["config"]["runner_seconds_per_tracker_rank0"] = {k: round(v["seconds"], 4) for k, v in runner.timings.items()}
                out["config"]["runner_host_tail_seconds_rank0"] = {k: round(v["host_tail_seconds"], 4) for k, v in runner.timings.items() if "host_tail_seconds" in v}
            if world > 1:
                # N > 1: the path BASELINE configs[3] names (reference trackers/runner.py:185-236 over ONE clip): a single clip
                # of world x K x B frames, TrackingRunner(distributed=True) — every rank runs the stateless part of each tracker
                # on its contiguous shard, the partials are gathered to rank 0 as packed arrays (dist.gather_arrays) and the
                # frame-sequential part (ByteTrack ids in global frame order, result containers) runs there.  Seconds = max
                # over ranks with the gathers and rank 0's sequential stages inside.  THIS is `value` at N > 1; the
                # independent-replica figure above (each rank its own runner over its own clip: an upper bound that omits the
                # gather and the rank-0 stage) stays beside it.
                if a.full:
                    out["replica_runners"] = {"value": out["value"], "ms_per_step": out["ms_per_step"],
                                              "what": "N independent TrackingRunner.run() over N private clips: no gather, ByteTrack per rank"}
                gclip = clip.alias(world * max(K, Wm, 1))       # rank r only ever reads frames [r K B, (r + 1) K B): its own
                if Wm > 0:
                    run_runner(gclip, world * Wm, distributed=True)
                dt, runner = run_runner(gclip, world * K, distributed=True)
                out["value"] = round(world * B * K / dt, 2)
                out["ms_per_step"] = round(1e3 * dt / K, 3)
                out["config"]["timed_path_n_gpus"] = "TrackingRunner(distributed=True), ONE clip of world x K x B frames: shards, packed gather to rank 0"
                out["config"]["runner_seconds_per_tracker_rank0"] = {k: round(v["seconds"], 4) for k, v in runner.timings.items()}
            if a.dump_outputs and rank == 0:
                # the last step = the last B frames of every rank's shard (at N > 1 rank 0 holds the merged results of all shards)
                write_outputs(a.dump_outputs, runner_outputs(trackers, [r * K * B + (K - 1) * B + i for r in range(world) for i in range(B)]))
            kept = sum(len(p) for p in trackers["players"].results.predictions) if "players" in trackers else 0
            out["config"]["tracked_players_rank0"] = kept
            out["config"]["frames_with_results_rank0"] = {n_: len(t_.results) for n_, t_ in trackers.items()}
        else:
            out["value"], out["ms_per_step"] = out["engine_only"]["value"], out["engine_only"]["ms_per_step"]
        T.set_eager_objects(False)          # (read by the containers' constructors alone: the count below is not affected)
        # how many result OBJECTS the timed run created (`Players` / `PlayersKeypoints` can keep the detector's arrays and build
        # their `Player` / `PlayerKeypoints` objects on first access; the reference — and `value` — build them eagerly,
        # players_tracker.py:371-378): count what the timed region materialised
        if a.full and not a.engine_only:
            om = {}
            for nm_, t_ in trackers.items():
                preds = t_.results.predictions
                cached = lambda p_: getattr(p_, "_players", None) if hasattr(p_, "_players") else getattr(p_, "_items", None)
                lazy = [p_ for p_ in preds if hasattr(p_, "_players") or hasattr(p_, "_items")]
                if not lazy:
                    om[nm_] = {"containers": len(preds), "array_backed": False}
                    continue
                inside = sum(len(cached(p_)) for p_ in lazy if cached(p_) is not None)
                t1_ = time.perf_counter()
                total = sum(len(p_.players) if hasattr(p_, "_players") else len(p_.players_keypoints) for p_ in lazy)
                om[nm_] = {"containers": len(preds), "array_backed": True, "objects_built_inside_timed_region": inside,
                           "objects_total": total, "build_all_ms": round(1e3 * (time.perf_counter() - t1_), 2)}
            out["objects_materialised"] = om
            if world == 1:
                run_runner(clip, 1)
                dt_lz, _ = run_runner(clip, K)
                out["value_lazy_objects"] = {"value": round(world * B * K / dt_lz, 2), "ms_per_step": round(1e3 * dt_lz / K, 3),
                                             "what": "the same run with Player / PlayerKeypoints objects left to first access (rounds 2-4's `value`)"}
        if not a.engine_only and not a.no_eager:
            # The reference builds every Player / PlayerKeypoints object inside predict_sample (players_tracker.py:371-378,
            # players_keypoints_tracker.py:303-320); `value` builds them on first access (none inside the timed region).  Same
            # run with the containers in eager mode: (i) on the timed checkpoints, whose class bias is calibrated so that ~1 %
            # of the anchors pass (hundreds of detections per frame: decode / NMS do real work, object construction is
            # unrepresentatively heavy); (ii) on a second calibration of the same graphs with a court-like handful of
            # detections per frame.
            def per_frame(trk):
                return {n_: round(sum(len(p_) for p_ in t_.results.predictions) / max(len(t_.results.predictions), 1), 2)
                        for n_, t_ in trk.items() if n_ != "ball"}
            T.set_eager_objects(2)                 # every object the reference allocates: the 13 PlayerKeypoint records per person too
            try:
                run_runner(clip, 1)
                dt_g, _ = run_runner(clip, K)
                ve = {"timed_checkpoints_all_records": {
                    "value": round(world * B * K / dt_g, 2), "ms_per_step": round(1e3 * dt_g / K, 3), "objects_per_frame": per_frame(trackers),
                    "what": "set_eager_objects(2): also the 13 PlayerKeypoint records of every person and their name index inside "
                            "predict_sample (Python dataclass construction: ~35 us per person, hundreds of persons per frame on these checkpoints)"}}
                T.set_eager_objects(True)
                if world == 1:
                    # second calibration of the SAME checkpoints: the class bias of every head is shifted so that, on the clip,
                    # ~6 candidates per frame pass `conf` (what a padel court shows: 4 players, the odd spectator) — the shift
                    # comes from the score distribution the engine itself reports at conf 0.01 (setup, untimed)
                    target = 6
                    sds = {}
                    for n_ in names:
                        cfg_ = TRACKERS[n_]
                        sd_ = dict(make_state_dict(n_, cfg_, frames))
                        bx, _, cn = trackers[n_].model._ensure_model().yolo_infer(
                            clip.buffer, B, H, W, imgsz=cfg_["imgsz"], conf=0.01, iou=0.7, classes=cfg_["classes"],
                            pre_mode=E.PRE_PIL_STRETCH if cfg_["pre"] == "pil" else E.PRE_LETTERBOX, channel_reverse=cfg_["rev"])
                        sc = np.sort(np.concatenate([bx[i, :cn[i], 4] for i in range(B)]))[::-1]
                        s_star = float(np.clip(sc[min(target * B, len(sc) - 1)], 1e-4, 1 - 1e-4)) if len(sc) else cfg_["conf"]
                        delta = np.log(cfg_["conf"] / (1 - cfg_["conf"])) - np.log(s_star / (1 - s_star))
                        for l in range(3):
                            k_ = f"model.22.cv3.{l}.2.bias"
                            b_ = np.asarray(sd_[k_], np.float32).copy()
                            b_[0] += np.float32(delta)
                            sd_[k_] = b_.astype(np.float16).astype(np.float32)
                        sds[n_] = sd_
                    def cls_shift(sd_, delta):
                        for l in range(3):
                            k_ = f"model.22.cv3.{l}.2.bias"
                            b_ = np.asarray(sd_[k_], np.float32).copy()
                            b_[0] += np.float32(delta)
                            sd_[k_] = b_.astype(np.float16).astype(np.float32)
                    with contextlib.redirect_stdout(sys.stderr):
                        rtrk, _ = build_trackers(names, frames, rank, B, H, W, eng, tmp, half=a.dtype == "f16", tag="_real",
                                                 replay=a.replay, sd_override=sds)
                        # one refinement on the recalibrated models themselves (the first estimate ranks NMS survivors of a
                        # 300-per-image list): the score of their own (target x B)-th detection becomes the new threshold
                        redo = False
                        for n_ in names:
                            cfg_ = TRACKERS[n_]
                            bx, _, cn = rtrk[n_].model._ensure_model().yolo_infer(
                                clip.buffer, B, H, W, imgsz=cfg_["imgsz"], conf=cfg_["conf"], iou=0.7, classes=cfg_["classes"],
                                pre_mode=E.PRE_PIL_STRETCH if cfg_["pre"] == "pil" else E.PRE_LETTERBOX, channel_reverse=cfg_["rev"])
                            if int(cn.sum()) > 2 * target * B:
                                sc = np.sort(np.concatenate([bx[i, :cn[i], 4] for i in range(B)]))[::-1]
                                s2 = float(np.clip(sc[target * B], 1e-4, 1 - 1e-4))
                                cls_shift(sds[n_], np.log(cfg_["conf"] / (1 - cfg_["conf"])) - np.log(s2 / (1 - s2)))
                                redo = True
                        if redo:
                            for t_ in rtrk.values():
                                t_.model.close()
                            rtrk, _ = build_trackers(names, frames, rank, B, H, W, eng, tmp, half=a.dtype == "f16", tag="_real2",
                                                     replay=a.replay, sd_override=sds)
                    T.set_eager_objects(False)
                    run_runner(clip, 1, trk=rtrk)
                    dt_l, _ = run_runner(clip, K, trk=rtrk)
                    T.set_eager_objects(True)
                    run_runner(clip, 1, trk=rtrk)
                    dt_r, _ = run_runner(clip, K, trk=rtrk)
                    ve["realistic_detections"] = {"value": round(world * B * K / dt_r, 2), "ms_per_step": round(1e3 * dt_r / K, 3),
                                                  "value_lazy_objects": round(world * B * K / dt_l, 2),
                                                  "objects_per_frame": per_frame(rtrk),
                                                  "what": "same graphs and weights, class bias of the heads shifted for ~6 detections per frame (a court's worth)"}
                    for t_ in rtrk.values():
                        t_.model.close()
            finally:
                T.set_eager_objects(False)
            ve["what"] = ("`value` builds Player / PlayerKeypoints inside predict_sample like the reference (array-backed); here: the same "
                          "with every per-keypoint record too, and — realistic_detections — on a court-like number of detections")
            out["value_eager_objects"] = ve
        if not a.no_host_frames and not a.engine_only:
            with video.ArrayClip(frames, repeat=max(K, 1)).pin(eng) as hclip:     # a decoder writing into page-locked memory
                run_runner(hclip, 1)
                dt_s, _ = run_runner(hclip, K)
                run_runner(hclip, 1, fanout=True, engine=eng)
                dt_f, _ = run_runner(hclip, K, fanout=True, engine=eng)
            out["host_frames"] = {"sequential_frames_per_s": round(world * B * K / dt_s, 2),
                                  "fanout_frames_per_s": round(world * B * K / dt_f, 2), "pinned": True,
                                  "what": "clip in page-locked host memory (hipHostRegister), PCIe-inclusive: one upload per "
                                          "tracker (reference order, runner.py:215-228) vs one upload per batch feeding all "
                                          "trackers (TrackingRunner(fanout=True)); never `value`"}
        if not a.no_reference_default and not a.engine_only and a.workload == "c3" and a.dtype == "f32":
            # the reference's ACTUAL default configuration: players yolov8m, pose @1280, and the TrackNetV3 ball tracker
            # (config.py:22,29-30,36-39; ball_tracker.py:373-523) instead of BASELINE's "ball YOLOv8 detect"
            from oracle import tracknet_ref as tr          # seeded synthetic TrackNet weights (setup only)
            from padel_analytics_amd import checkpoint
            from padel_analytics_amd.trackers import BallTracker
            tpath = Path(tmp) / f"tracknet_r{rank}.pt"
            checkpoint.save_checkpoint(tpath, tr.synth_tracknet_state_dict(3), "tracknet", param_dict={"seq_len": 8, "bg_mode": "concat"})
            # (background median over the first B frames: the HBM-resident clip is B distinct frames repeated K times, so
            #  the reference's 1800-frame window would see the same B frames over and over)
            ipath = Path(tmp) / f"inpaintnet_r{rank}.pt"
            checkpoint.save_checkpoint(ipath, tr.synth_inpaintnet_state_dict(4), "inpaintnet", param_dict={"seq_len": 16})
            bt = BallTracker(str(tpath), str(ipath), batch_size=B, median_max_sample_num=B)
            bt._engine = eng
            ref_trackers = [trackers["players"], trackers["pose"], bt]

            def run_ref(n_batches):
                runner = TrackingRunner(ref_trackers, clip, Path(tmp) / "out_ref.mp4", start=0, end=n_batches * B)
                runner.restart()
                fence()
                t0_ = time.perf_counter()
                runner.run()
                fence()
                return eng.allreduce_max(time.perf_counter() - t0_), runner

            run_ref(1)
            dt_r, rr = run_ref(K)
            out["reference_default"] = {
                "value": round(world * B * K / dt_r, 2), "unit": "frames/s", "ms_per_step": round(1e3 * dt_r / K, 3),
                "trackers": {"players": "yolov8m-detect-nc80 @640 + PolygonZone + ByteTrack", "pose": "yolov8m-pose13x3 @1280",
                             "ball": "TrackNetV3 27->8 @288x512, one window per frame, median background over the clip, "
                                     "temporal ensemble, threshold, connected components on the device, InpaintNet trajectory repair over "
                                     "the whole clip (device network, host windows / blending) (BallTracker)"},
                "conv_gflop_per_frame": round((flops_per_frame["players"] + flops_per_frame["pose"]) / 1e9 + 227.61, 1),
                "seconds_per_tracker_rank0": {k_: round(v_["seconds"], 4) for k_, v_ in rr.timings.items()},
                "what": "TrackingRunner.run() over the same HBM-resident clip with the reference's default trackers"}
            bt.to("cpu")

    if rank == 0 and not a.no_roofline:
        # ---- roofline of the dominant kernel (conv3x3 implicit GEMM, fp32 MFMA): HIP events recorded on
        # the engine's own stream around every launch of one extra (untimed) engine step
        eng.set_profiling(True)
        engine_step()
        recs = []
        for name in names:
            recs += trackers[name].model._model.last_profile()
        eng.set_profiling(False)
        if a.dump_ops:
            with open(a.dump_ops, "w") as f:
                f.write("tracker,kind,ksize,M,cout,cin,stride,bm,bn,ms,flops,res\n")
                for name in names:
                    for r in trackers[name].model._model.profile_rows():
                        f.write(f"{name},{r['kind']},{r['ksize']},{r['M']},{r['cout']},{r['cin']},{r['stride']},"
                                f"{r['mf']},{r['nf']},{r['ms']:.5f},{r['flops']:.0f},{r.get('res', 0)}\n")
        c3 = [r for r in recs if r["kind"] == 2 and r["ksize"] == 3]
        c1 = [r for r in recs if r["kind"] == 2 and r["ksize"] == 1]
        ms3, fl3 = sum(r["ms"] for r in c3), sum(r["flops"] for r in c3)
        ms1, fl1 = sum(r["ms"] for r in c1), sum(r["flops"] for r in c1)
        ms_all = sum(r["ms"] for r in recs)
        ach = fl3 / (ms3 * 1e-3) / 1e12 if ms3 > 0 else 0.0
        PEAK = PEAK_FP16_MFMA_TFLOPS if a.dtype == "f16" else PEAK_BY_IMPL[a.impl]
        # h2: MFMA products per multiply actually ISSUED — 3, or 2 on convs whose packed weights have an all-zero correction plane
        # (PA_CONV_W_SINGLE: fp16 checkpoint weights, BatchNorm's scale in the output scale).  FLOP-weighted over the graphs;
        # the fp32-equivalent peak of the f16 pipe is 2500 / that, so that `frac` stays what it was: matrix-pipe utilisation
        prod = {3: 3.0, 1: 3.0}
        if a.dtype == "f32" and a.impl == "h2":
            from padel_analytics_amd import graph as G_
            for ks in (3, 1):
                num = den = 0.0
                for name in names:
                    g_ = trackers[name].model._model.graph
                    for o_ in g_.ops:
                        if o_["kind"] == G_.OP_CONV and o_["ksize"] == ks:
                            w_ = float(o_["cout"]) * o_["cin"] * ks * ks / 4.0 ** g_.bufs[o_["out_buf"]][0] * flops_per_frame[name] / max(g_.conv_flops(64, 64), 1.0)
                            num += w_ * (2.0 if (o_.get("flags", 0) & 1) else 3.0)
                            den += w_
                prod[ks] = num / den if den else 3.0
            PEAK = round(PEAK_FP16_MFMA_TFLOPS / prod[3], 1)
        PEAK1 = round(PEAK_FP16_MFMA_TFLOPS / prod[1], 1) if (a.dtype == "f32" and a.impl == "h2") else PEAK
        traffic = None
        # PMC FETCH_SIZE / WRITE_SIZE passes over this script's own engine-only step (measure_traffic); when rocprofv3 is not
        # available (or --traffic static) the committed measurement of the same command line, marked "static"
        if a.dtype == "f32" and a.traffic == "live" and world == 1:
            os.environ.setdefault("PADEL_BENCH_SD_CACHE", str(tmp))
            rows_all = []
            for name in names:
                rows_all += trackers[name].model._model.profile_rows()
            with contextlib.redirect_stdout(sys.stderr):
                traffic = measure_traffic(a, rows_all, tmp)
        tpath = ROOT / "profiles" / "r6_traffic.json"
        if traffic is None and a.traffic != "none" and tpath.exists():
            tj = json.loads(tpath.read_text()).get(f"{a.workload}-{a.impl}" if a.dtype == "f32" else "none")
            if tj:
                traffic = {"bytes_per_launch": tj["bytes_per_launch"], "fetch_bytes_per_launch": tj["fetch_bytes_per_launch"],
                           "write_bytes_per_launch": tj["write_bytes_per_launch"],
                           "algorithmic_bytes_per_launch": tj["algorithmic_bytes_per_launch"],
                           "ratio_to_algorithmic": tj.get("ratio_to_algorithmic"), "static": True,
                           "source": ("profiles/r6_traffic.json: " + tj["source"])[:118]}
        out["roofline"] = {
            "kernel": ("conv_p16 / conv_p16q (stride-1 3x3 patch kernels) + conv_tap16 (stride 2); v_mfma_f32_16x16x32_f16" if a.dtype == "f16" else
                       "conv_h2r / h2q / h2p / h2w (stride-1 3x3 patch kernels) + conv_h2 (stride 2); 2-3 x v_mfma_f32_16x16x32_f16 per block" if a.impl == "h2" else
                       "conv_bx3p (stride-1 3x3 patch) + conv_bx3 (stride 2); exact bf16x3, 6 x v_mfma_f32_16x16x32_bf16 per block" if a.impl == "bx3" else
                       "conv_tap_kernel (3x3 implicit GEMM, LDS-DMA ring, v_mfma_f32_16x16x4_f32)"),
            "peak_note": ("fp32-eq peak = 2500 / MFMA products per multiply (2 on fp16-number weights, else 3); frac = matrix-pipe utilisation"
                          if (a.dtype == "f32" and a.impl == "h2") else
                          "fp32-eq peak = bf16 MFMA dense 2500 / 6 products per multiply; the fp32-input MFMA peak is 157.3"
                          if (a.dtype == "f32" and a.impl == "bx3") else None),
            "bound": "mfma", "achieved": round(ach, 2), "peak": PEAK, "unit": "TFLOP/s",
            "frac": round(ach / PEAK, 4), "traffic": traffic if a.dtype == "f32" else None,
            # whole-step number north_star asks for ("frames/s as fraction of the conv roofline"): every conv FLOP of the step over the
            # HEADLINE step time (runner, objects included) against the FLOP-weighted peak of the products issued
            "frac_whole_step": None,
            "traffic_ratio": (traffic or {}).get("ratio_to_algorithmic") if a.dtype == "f32" else None,
            "mfma_util_dominant": PMC_SUMMARY.get("mfma_util_dominant"), "mfma_util_source": PMC_SUMMARY.get("source"),
            "products_per_multiply": ({"conv3x3": round(prod[3], 3), "conv1x1": round(prod[1], 3)} if (a.dtype == "f32" and a.impl == "h2") else None),
            "frac_of_three_product_peak": (round(ach / PEAK_H2_TFLOPS, 4) if (a.dtype == "f32" and a.impl == "h2") else None),
            # what a kernel of nothing but v_mfma_f32_16x16x32_f16 (or 32x32x16) sustains on this chip with random operands (clock
            # under matrix load; 2.2-2.5 PFLOP/s with all-zero operands, 2.5 nominal): tools/mfma_f16_ubench.hip, a static figure
            "sustained_mfma_peak": ({"value": round(SUSTAINED_FP16_MFMA_TFLOPS / (prod[3] if a.dtype == "f32" else 1.0), 1), "unit": "TFLOP/s",
                                     "frac": round(ach / (SUSTAINED_FP16_MFMA_TFLOPS / (prod[3] if a.dtype == "f32" else 1.0)), 4), "static": True,
                                     "source": "profiles/r4a_mfma_f16_ubench.txt: 1.71-1.85 PFLOP/s of f16 MFMA on random operands"}
                                    if (a.dtype == "f16" or a.impl == "h2") else None),
            "launches": len(c3), "avg_launch_ms": round(ms3 / max(len(c3), 1), 4),
            "flops_per_step": fl3, "kernel_ms_per_step": round(ms3, 3),
            "conv1x1": conv1x1_roofline([r for name in names for r in trackers[name].model._model.profile_rows() if r["kind"] == 2 and r["ksize"] == 1],
                                        fl1, ms1, PEAK1, a),
            "all_kernels_ms_per_step": round(ms_all, 3),
            "other_ms_per_step": {str(k): round(sum(r["ms"] for r in recs if r["kind"] == k), 3)
                                  for k in sorted({r["kind"] for r in recs}) if k != 2},
        }
        prod_all = (fl3 * prod[3] + fl1 * prod[1]) / max(fl3 + fl1, 1.0) if (a.dtype == "f32" and a.impl == "h2") else None
        peak_all = (PEAK_FP16_MFMA_TFLOPS / prod_all) if prod_all else PEAK
        if out.get("ms_per_step"):
            out["roofline"]["frac_whole_step"] = round((fl3 + fl1) / (out["ms_per_step"] * 1e-3) / 1e12 / peak_all, 4)
            out["roofline"]["conv_tflop_per_step"] = round((fl3 + fl1) / 1e12, 3)
        m0 = trackers[names[-1]].model._model
        arena, logical = m0.plan_bytes()
        out["config"]["activation_arena_gib"] = {"tracker": names[-1], "allocated": round(arena / 2**30, 2),
                                                 "logical_buffers": round(logical / 2**30, 2)}

    if rank == 0 and not a.no_cpu_baseline and world == 1:
        # ---- CPU leg: the oracle (a restatement, kind "port") on this box's host cores, on a bounded sample of the
        # same workload: its time is the cpu_baseline, its outputs are the parity reference for the engine's
        # results on the same frames (box / keypoint L-inf in source pixels after NMS — BASELINE's "L-inf vs ref")
        from oracle import yolov8_ref as ref
        from tests import parity
        # 64 torch threads: more (this box has 256 hardware threads) only adds barrier cost on these
        # batch-2 graphs (measured: 256 threads -> 90 s/frame)
        ncores = min(os.cpu_count() or 1, 64)
        torch.set_num_threads(ncores)
        ns = 2                                      # parity sample (fp32 and fp64 oracle)
        nt = max(ns, (a.cpu_sample or 16) // ns * ns)     # timed sample of the CPU baseline: 16 frames = ~18 s of CPU work on the box's 64 threads for c3
        sample = frames[:ns]
        tcpu = 0.0
        if a.dtype != "f32":
            a.no_fp64 = True
        par = {"linf_px_vs_fp32_oracle": 0.0, "linf_px_vs_fp64": 0.0 if not a.no_fp64 else None,
               "oracle_floor_px": 0.0 if not a.no_fp64 else None, "classes_equal": True, "detection_sets_equal": True,
               "detections": 0, "per_tracker": {}, "frames": ns,
               "bar": "north_star: <= 1e-3 px; tests: engine-vs-fp64 <= max(1e-3, 4 x oracle floor), RMS <= 1.5 x floor (DESIGN.md 4)"}
        for name in names:
            cfg = TRACKERS[name]
            sd = make_state_dict(name, cfg, frames)       # same weights as the GPU run (deterministic)
            model = ref.YoloV8Ref(sd, cfg["nc"], cfg["kpt"])
            srcs = source_for_oracle(cfg, sample)
            ref.predict(model, source_for_oracle(cfg, sample[:1]), cfg["conf"], 0.7, cfg["imgsz"], cfg["classes"])  # warm
            t1 = time.perf_counter()
            # host-side processor (BGR2RGB / PIL resize) + predict, like predict_sample() times it
            r32 = ref.predict(model, source_for_oracle(cfg, sample), cfg["conf"], 0.7, cfg["imgsz"], cfg["classes"])
            tcpu += time.perf_counter() - t1
            # the TIMED sample is larger than the parity sample (2 frames are a tiny baseline): nt frames in passes
            # of ns, ~18 s of CPU work on the box's EPYC for c3 (round 4: 8 frames, 9 s); the parity statements stay on the first ns frames (their
            # fp64 evaluation is 3-4 x slower)
            for lo in range(ns, nt, ns):
                t1 = time.perf_counter()
                ref.predict(model, source_for_oracle(cfg, frames[lo:lo + ns]), cfg["conf"], 0.7, cfg["imgsz"], cfg["classes"])
                tcpu += time.perf_counter() - t1
            # engine results on the same frames (B = 64 pass; bitwise equal to any other batch size —
            # tests/test_gpu_bench_config.py::test_batch_invariance)
            boxes, kpts, counts = trackers[name].model._ensure_model().yolo_infer(
                clip.buffer, B, H, W, imgsz=cfg["imgsz"], conf=cfg["conf"], iou=0.7, classes=cfg["classes"],
                pre_mode=E.PRE_PIL_STRETCH if cfg["pre"] == "pil" else E.PRE_LETTERBOX, channel_reverse=cfg["rev"])
            boxes, counts = boxes[:ns], counts[:ns]
            kpts = None if kpts is None else kpts[:ns]
            entry = {}
            if a.dtype != "f32":
                # reduced precision: detection sets may differ near the thresholds; report how many of the oracle's
                # detections the path reproduces and its own L-inf on those (no parity claim for this dtype)
                tot = mt = 0
                worst = 0.0
                for i, r in enumerate(r32):
                    gb = boxes[i, :counts[i]]
                    pairs, ru, gu = parity.match(r["boxes"], gb, tol_match=8.0)
                    tot += len(r["boxes"]); mt += len(pairs)
                    for i_r, i_g in pairs:
                        worst = max(worst, float(np.abs(gb[i_g, :4] - r["boxes"][i_r, :4]).max()))
                        if kpts is not None and r["kpts"] is not None:
                            gk = kpts[i, i_g].reshape(*cfg["kpt"])
                            worst = max(worst, float(np.abs(gk[..., :2] - r["kpts"][i_r][..., :2]).max()))
                entry.update(detections=tot, matched=mt, linf_px_vs_fp32_oracle=round(worst, 4))
                par["linf_px_vs_fp32_oracle"] = max(par["linf_px_vs_fp32_oracle"], worst)
                par["detections"] += tot
                par["detection_sets_equal"] = par["detection_sets_equal"] and mt == tot == int(counts.sum())
                par["per_tracker"][name] = entry
                continue
            try:
                g32 = parity.compare_batch(r32, boxes, kpts, counts, cfg["conf"], 0.7, kpt_shape=cfg["kpt"])
                entry.update(detections=g32["n"], linf_px_vs_fp32_oracle=g32["worst_px"], rms_px_vs_fp32_oracle=g32["rms_px"],
                             score_err=g32["worst_score"], flips=len(g32["flips"]))
                par["linf_px_vs_fp32_oracle"] = max(par["linf_px_vs_fp32_oracle"], g32["worst_px"])
                par["detections"] += g32["n"]
                if not a.no_fp64:
                    r64 = ref.predict(ref.YoloV8Ref(sd, cfg["nc"], cfg["kpt"], dtype=torch.float64), srcs, cfg["conf"], 0.7,
                                      cfg["imgsz"], cfg["classes"])
                    nk = 0 if cfg["kpt"] is None else cfg["kpt"][0] * cfg["kpt"][1]
                    b64 = np.zeros((ns, 300, 6), np.float32)
                    k64 = np.zeros((ns, 300, nk), np.float32) if nk else None
                    c64 = np.zeros(ns, np.int32)
                    for i, r in enumerate(r64):
                        c64[i] = len(r["boxes"])
                        b64[i, :c64[i]] = r["boxes"]
                        if nk and c64[i]:
                            k64[i, :c64[i]] = r["kpts"].reshape(c64[i], -1)
                    floor = parity.compare_batch(r32, b64, k64, c64, cfg["conf"], 0.7, kpt_shape=cfg["kpt"])
                    g64 = parity.compare_batch(r64, boxes, kpts, counts, cfg["conf"], 0.7, kpt_shape=cfg["kpt"])
                    entry.update(linf_px_vs_fp64=g64["worst_px"], oracle_floor_px=floor["worst_px"],
                                 rms_px_vs_fp64=g64["rms_px"], rms_floor_px=floor["rms_px"])
                    par["linf_px_vs_fp64"] = max(par["linf_px_vs_fp64"], g64["worst_px"])
                    par["oracle_floor_px"] = max(par["oracle_floor_px"], floor["worst_px"])
            except AssertionError as e:                    # class ids / detection sets differ: report, do not hide
                par["classes_equal"] = par["detection_sets_equal"] = False
                entry["mismatch"] = str(e)[:300]
            par["per_tracker"][name] = {k: (round(v, 6) if isinstance(v, float) else v) for k, v in entry.items()}
        for k in ("linf_px_vs_fp32_oracle", "linf_px_vs_fp64", "oracle_floor_px"):
            if par[k] is not None:
                par[k] = round(par[k], 6)
        if a.dtype == "f32" and not a.no_fp64 and not a.no_tight:
            par["low_noise_heads"] = parity_low_noise_heads(eng, names, frames, sample, H, W, ref, parity)
        out["parity"] = par
        out["config"]["parity_linf_px_vs_fp32_oracle"] = par["linf_px_vs_fp32_oracle"]
        out["config"]["parity_oracle_floor_px"] = par["oracle_floor_px"]
        out["config"]["parity_linf_px_vs_fp64"] = par["linf_px_vs_fp64"]
        if isinstance(par.get("low_noise_heads"), dict):
            out["config"]["parity_low_noise_linf_px"] = par["low_noise_heads"].get("linf_px_vs_fp32_oracle")
        out["cpu_baseline"] = {"value": round(nt / tcpu, 3), "unit": "frames/s", "cores": ncores, "kind": "port", "seconds": round(tcpu, 2),
                               "sample": f"{nt} frames of the workload ({tcpu:.1f} s) through oracle/yolov8_ref.py, {len(names)} trackers, {ncores} torch threads"}

    if a.dtype == "f32" and a.impl == "h2" and not a.no_compare and world == 1:
        # the strict-fp32 number beside `value`; last, because it rebuilds the trackers' graphs on fp32 storage
        with contextlib.redirect_stdout(sys.stderr):
            out["engine_only"]["fp32_mfma_kernels"] = fp32_mfma_leg()
            out["config"]["fp32_strict_frames_per_s"] = out["engine_only"]["fp32_mfma_kernels"]["value"]

    if fake is not None:
        # test hook: what every rank's models saw (weights only through the broadcast on ranks != 0) and computed
        mine = {"rank": rank, "log": list(fake.LOG),
                "weight_checksums": {n_: t_.model._ensure_model().weight_checksum() for n_, t_ in trackers.items()},
                "first_boxes": {n_: [round(float(v), 3) for v in t_.model._ensure_model().yolo_infer(
                    clip.buffer.view(0, clip.frame_bytes), 1, H, W, imgsz=TRACKERS[n_]["imgsz"], conf=TRACKERS[n_]["conf"], iou=0.7)[0][0, 0, :4]]
                    for n_, t_ in trackers.items()}}
        allr = D.gather_results([mine], dst=0)
        if rank == 0:
            out["fake_engine"] = True
            out["ranks"] = allr

    if rank == 0:
        # the driver's record keeps top-level scalars, `config`, `roofline`, `cpu_baseline` and cuts strings at ~128 characters: none of
        # ours may be longer than 120 there — reported, not silently cut
        def long_strings(o, path, acc):
            if isinstance(o, dict):
                for k_, v_ in o.items():
                    long_strings(v_, f"{path}.{k_}" if path else str(k_), acc)
            elif isinstance(o, str) and len(o) > 120:
                acc.append(path)
            return acc
        too_long = long_strings({k_: v_ for k_, v_ in out.items() if k_ in ("config", "roofline", "cpu_baseline") or not isinstance(v_, (dict, list))}, "", [])
        if too_long:
            out["strings_over_120_chars"] = too_long
            print("bench: strings longer than 120 characters in kept fields: " + ", ".join(too_long), file=sys.stderr)
        with os.fdopen(json_fd, "w") as f:
            f.write(json.dumps(out) + "\n")
    for t in trackers.values():
        t.model.close()
    clip.free()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
