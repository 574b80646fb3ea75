"""TrackingRunner — drop-in for the tracker loop of the reference's ``trackers/runner.py``
(``__init__`` :37-79, ``run`` :175-236): trackers run one after the other over the whole clip, each is
moved to the device, timed with ``timeit`` exactly where the reference times it (:222-228), moved back,
and its predictions are cached as JSON; a tracker with cached predictions is skipped (:187-191).

Additions (all off by default, the reference's sequential semantics stay the default):

* ``run()`` records ``self.timings`` (seconds / frames per tracker) and prints frames/s;
* ``distributed=True``: one process per GPU under ``torch.distributed``; every tracker's frames
  are split into contiguous shards ``dist.shard_range`` (plus the tracker's ``temporal_context`` — TrackNet's 7-frame
  halo), each rank runs the stateless part on its shard (``Tracker.predict_partial``), the per-frame partials are
  gathered to rank 0 in frame order and the sequential part (ByteTrack ids, InpaintNet) runs there
  (``Tracker.merge_partials``).  The ball tracker's background median is computed once on rank 0 and broadcast.
  Results and JSON caches live on rank 0;
* ``fanout=True``: ONE pass over the video feeds every tracker — each batch of frames is
  uploaded to HBM once (the next batch uploads on the engine's copy stream while this one computes) and all
  batch trackers consume the same device-resident frames; stream trackers (TrackNet) get the same handles.  The
  reference decodes and uploads the clip once per tracker (:215-220).

* ``render=`` a path or a ``video.FrameSink`` (``.avi`` / ``.mjpeg`` / ``.mjpg``: Motion-JPEG of ``render_quality``, encoded on the GPU
  — ``video.MjpegSink``; any other path: ``.y4m``): ``draw_and_collect_data`` (reference :91-173) reads the clip again and writes it
  with every tracker's results drawn on it — on the GPU (csrc/render.hip: marks applied to the BGR frames in HBM and converted to
  YUV 4:2:0 in one pass), one download and one write per batch.  Without it (the default) the step prints that it is skipped;
  ``render_scale=`` 2, 3 or 4 writes the clip at 1 / render_scale of the source's size, every pixel the rounded mean of the rendered
  source pixels under it, in that same pass (``pa_render_scaled``): an anti-aliased copy of 1 / render_scale² the bytes — and the way
  to an ``.avi`` of a clip wider than the JPEG encoder's 2560.  Marks, the inset and the collected data stay in source pixels.  A
  scale the clip's size does not allow, or a ``FrameSink`` of another size than the rendered frames, is a ``ValueError`` in ``__init__``;
* ``topdown=`` a path or a ``video.FrameSink``, as for ``render=``: a second clip, every frame warped through its court homography into
  a metric canvas of the court (``topdown.TopDownView``; ``topdown_options``: its keyword arguments ``px_per_m``, ``margin_m``, ``fill``) —
  ``Engine.warp`` (csrc/warp.hip) into a BGR canvas in HBM, then ``Engine.render`` of that canvas with the court's lines, the players
  and the ball as marks.  The real footage seen from above: whether the floor, rectified, looks like a padel court is the check of
  the homography the inset cannot give.  It shares the walk over the clip with ``render=`` when both are given, follows ``segments=``
  as ``render=`` does, is rank 0's under ``distributed``, and ignores ``render_scale``; ``render_quality`` serves both files.  A frame
  without a homography is ``fill`` with ``NO COURT`` on it.  ``ValueError`` in ``__init__``: no tracker gives ``Keypoints``, a canvas the
  sink refuses, a ``FrameSink`` of another size than the canvas, ``fanout=True``.  ``timings["__topdown__"]``: seconds, frames, bytes;

* ``heatmap=`` a path ending in ``.npy`` or ``.jpg``: where on the court each player spent the clip (``heatmap.HeatMap``; ``heatmap_options``:
  its keyword arguments ``radius_m``, ``saturate_s``, ``alpha``, ``ids``, ``show``, and ``overlay``) — one density map per player id on the
  top-down canvas (``topdown_options`` size it, with or without ``topdown=``), an Epanechnikov bump per frame under each player's feet.
  ``.npy``: the final maps, (planes, h, w) uint32.  ``.jpg``: one picture, the maps blended over a ``fill`` canvas at ``full`` = their
  largest density, the court's lines over it, made by the renderer and the JPEG encoder.  With ``topdown=`` every canvas batch gets one
  ``Engine.heat`` (csrc/heat.hip) between the warp and the canvas render: the clip shows the map growing under the players
  (``overlay=False``: accumulated, not shown).  Without ``topdown=`` the maps come from the stored results alone
  (``heatmap.accumulate_host``): no frame is read for them, no GPU touched.  ``heat_state`` holds the final maps,
  ``timings["__heatmap__"]`` the step's seconds and frames.  After ``identities=True``, so the planes are the relabelled ids; follows
  ``segments=`` and ``distributed`` as ``topdown=`` does.  ``ValueError`` in ``__init__``: no tracker gives ``Keypoints``, none gives
  ``Players``, ``fanout=True``, another suffix, an unknown or refused option.  The defaults are parameters, not findings;

* ``collect_data=True`` (the reference's own switch, :74-79): the step also projects every frame's players and ball into the 2-D
  court (``projected_court.ProjectedCourt.project_batch``: the reference's homography state machine :633-647, the frames of a batch
  that need a homography solved together) and fills ``self.data_analytics`` (``analytics.DataAnalytics``) with the players' positions
  in metres, frame by frame in the reference's order (:139-167) — the hand-over of its ``main.py``,
  ``runner.data_analytics.into_dataframe(fps)``.  With ``render`` the court inset is drawn too (``court_inset``: None = "iff
  ``collect_data``"): the translucent panel — the renderer's one blending mark — the court, and the projected players and ball.
  Without ``render`` the data are collected from the stored results alone: no frame is read, no GPU touched.  ``timings["__collect__"]``
  is the host time of projection and collection.  Under ``distributed`` all of it is rank 0's.

* ``segments=`` (the reference's open item, ``main.py:122``: "FILTER FRAMES OF INTEREST"): the trackers and the render step see only
  the frames of some half-open ranges ``(lo, hi)`` of source frame numbers — a list, or ``"court"``: ``activity.scan`` +
  ``court_view_mask`` + ``segments`` over [start, end) before the first tracker (``segment_options``: keyword arguments for them;
  ``timings["__segments__"]``).  ``source_index[i]`` is the source frame of kept position ``i``; ``n_available``, ``total_frames``,
  every tracker's ``results`` and ``Ball.frame`` count kept frames.  Each tracker runs segment by segment, in order: no batch (and no
  TrackNet window, no InpaintNet sequence) spans a cut, while ByteTrack and every other state a tracker keeps between batches carry
  over.  A stream tracker's background is computed once, over the first kept frames.  ``DataAnalytics`` deltas across a cut are not
  corrected.  Not with ``distributed`` or ``fanout``.

* ``identities=True``: ByteTrack never gives a lost track its old id back, so a player who was hidden for longer than its buffer
  returns as id 5, 6, ... and ``DataAnalytics`` drops them.  After the trackers (and after their prediction caches are written:
  the caches keep ByteTrack's ids, so a cached run gives the same answer as a fresh one) and before ``draw_and_collect_data``, the
  stored boxes of the tracker whose ``object()`` is ``Players`` get colour histograms in a second pass over the kept frames
  (``identity.scan``: csrc/box_histogram.hip), ``identity.assign`` maps the tracks to four identities, and that tracker's results are
  replaced in memory by ``Players`` with the mapped ids (``identity.relabel``).  ``identity_options``: ``every``, ``batch``,
  ``on_device`` for the scan, ``n_players``, ``max_distance`` for the assignment.  ``identity_map`` is the mapping,
  ``identity_distances`` what it was decided by, ``timings["__identities__"]`` the pass.  The thresholds are parameters, not
  findings.  Not with ``distributed`` or ``fanout``.

* ``ball_trail=N`` (the reference's ``draw_multiple_frames``, ``ball_tracker.py:324-347``, which its runner never calls): the render
  step also draws where the ball was seen in the last N kept frames, the current one included (``trail_marks``); a trail does not
  reach across a cut of ``segments``.  0, the default, draws none."""
from __future__ import annotations

import os
import timeit
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from pathlib import Path
from typing import Callable, Optional

import numpy as np

from .. import dist as D, video
from . import outputs as O
from .tracker import NoPredictFrames, Tracker, _sampler, host_stages, relaxed_gc


@dataclass(eq=False)
class _Deferred:
    """What ``run()`` owes a tracker from the start of its loop on: the wait for its work that finishes later, the report, the save."""
    tracker: Tracker
    wait: Optional[Callable] = None    # None: nothing is outstanding; else -> None, or the (start, end) span of the work
    t0: Optional[float] = None         # the tracker's loop as run() times it (t1 None: the loop did not end)
    t1: Optional[float] = None
    merge: bool = False                # rank 0's sequential stage on the merge thread (else: the queued host stages of a batch loop)
    overlapped: bool = False           # another tracker's loop ran after this was registered


class TrackingRunner:
    def __init__(self, trackers: list, video_path: str | Path, inference_path: str | Path, start: int = 0,
                 end: Optional[int] = None, collect_data: bool = False, *, distributed: bool = False,
                 fanout: bool = False, engine=None, host_queue_depth: Optional[int] = None, render=None,
                 court_inset: Optional[bool] = None, render_quality: int = 90, segments=None,
                 segment_options: Optional[dict] = None, identities: bool = False, identity_options: Optional[dict] = None,
                 ball_trail: int = 0, render_scale: int = 1, topdown=None, topdown_options: Optional[dict] = None,
                 heatmap=None, heatmap_options: Optional[dict] = None) -> None:
        if isinstance(render_scale, bool) or render_scale not in (1, 2, 3, 4):
            raise ValueError(f"render_scale={render_scale!r}: 1, 2, 3 or 4 (the rendered clip at 1 / render_scale of the source's size)")
        self.render_scale = int(render_scale)
        self.video_path = video_path
        self.inference_path = inference_path
        self.start = start
        self.stride = 1
        self.end = end
        self.video_info = video.VideoInfo.from_video_path(video_path)
        self.total_frames = self.video_info.total_frames if end is None else end - start
        # frames actually available from `start` on (the reference reports the whole clip's length when end is None,
        # runner.py:52; the sharded path must split what the generator really yields)
        # (an `end` beyond the clip is clamped: the shards must add up to what the generator yields, or the last ranks come
        # up short and the others wait in the gather for ever)
        self.n_available = max(0, (self.video_info.total_frames if end is None else min(end, self.video_info.total_frames)) - start)
        self.trackers = {}
        for tracker in trackers:
            self.trackers[str(tracker)] = tracker.video_info_post_init(self.video_info)
        # reference :59-79: fixed keypoints keep the first homography for the whole clip
        from ..projected_court import ProjectedCourt
        from ..analytics import DataAnalytics
        self.is_fixed_keypoints = getattr(O.tracker_of(trackers, "Keypoints"), "fixed_keypoints_detection", None) is not None
        self.projected_court = ProjectedCourt(self.video_info)
        self.collect_data = collect_data
        self.data_analytics = DataAnalytics() if collect_data else None
        self.court_inset = bool(collect_data) if court_inset is None else bool(court_inset)   # None: on iff collect_data
        if collect_data:
            print("runner: Ready for data collection" + (" (fixed court keypoints)" if self.is_fixed_keypoints else ""))
        self.timings: dict = {}
        self.distributed = distributed
        self.fanout = fanout
        self.engine = engine
        # host stages (zone, ByteTrack, result objects) a batch tracker may have queued behind its device stage; what is still
        # queued when its device loop ends drains beside the NEXT tracker's device work (1: the loop waits for its own tail)
        self.host_queue_depth = int(os.environ.get("PADEL_HOST_QUEUE_DEPTH", 8)) if host_queue_depth is None else host_queue_depth
        self._deferred: list = []          # _Deferred, in tracker order: what run() has not reported and saved yet
        self._merge_pool = None            # sharded mode, rank 0: the thread of the sequential stages (created with the first one)
        self.render = render               # None | path of the file to write (.avi / .mjpeg / .mjpg: Motion-JPEG; anything else: .y4m) | video.FrameSink
        self.render_quality = int(render_quality)   # JPEG quality of a Motion-JPEG file (1..100)
        self.topdown = topdown             # None | path (suffixes as for render) | video.FrameSink: the clip seen from above
        self.heatmap = heatmap             # None | path ending in .npy (the final maps) or .jpg (a picture of them)
        self.heat_state: Optional[np.ndarray] = None   # the final maps, (planes, h, w) uint32: draw_and_collect_data
        # the outputs check themselves now: a ValueError costs no tracker run and leaves no file
        self._outputs = out = O.OutputStep(self, trackers, topdown_options, heatmap_options)
        self.topdown_view = out.top.view if out.top is not None else None        # topdown.TopDownView: the canvas
        self.heat = out.maps.heat if out.maps is not None else None              # heatmap.HeatMap: the parameters of the maps
        # kept frames: None = all of [start, start + n_available); else [(lo, hi)] source frame numbers, set by _set_segments
        self.segments: Optional[list] = None
        self._run_range = (self.start, self.start + self.n_available)      # the source frames this run may keep
        self.source_index = np.arange(self.start, self.start + self.n_available, dtype=np.int64)
        self.segment_options = dict(segment_options or {})
        self._segments_pending = False             # "court": resolved by run() before the first tracker (resolve_segments)
        if segments is not None:
            if distributed or fanout:
                raise ValueError("segments= is not available with distributed=True or fanout=True")
            if isinstance(segments, str):
                if segments != "court":
                    raise ValueError(f"segments={segments!r}: a list of (lo, hi) source frame numbers or \"court\"")
                self._segments_pending = True
            else:
                self._set_segments(segments)
        self.identities = bool(identities)
        self.identity_options = dict(identity_options or {})
        self.identity_map: Optional[dict] = None       # {ByteTrack id: id 1..4, or 5.. for a track nobody claimed}: repair_identities
        self.identity_distances: Optional[dict] = None
        if self.identities and (distributed or fanout):
            raise ValueError("identities=True is not available with distributed=True or fanout=True")
        self.ball_trail = int(ball_trail)              # kept frames whose ball positions frame_marks draws as a trail (0: none)
        if self.ball_trail < 0:
            raise ValueError(f"ball_trail={ball_trail!r}: a number of frames, 0 or more")

    def _set_segments(self, segments) -> None:
        """``segments``: ascending, non-overlapping, non-empty (lo, hi) inside [start, start + n_available) — else ``ValueError``
        naming the pair."""
        lo_all, hi_all = self._run_range
        segs, last = [], lo_all
        for pair in segments:
            lo, hi = (int(v) for v in pair)
            if hi <= lo:
                raise ValueError(f"segments: ({lo}, {hi}) is empty")
            if lo < lo_all or hi > hi_all:
                raise ValueError(f"segments: ({lo}, {hi}) leaves the frames [{lo_all}, {hi_all}) of this run")
            if lo < last:
                raise ValueError(f"segments: ({lo}, {hi}) starts before the end of the one in front of it ({last}): they must be "
                                 f"ascending and must not overlap")
            segs.append((lo, hi))
            last = hi
        self.segments = segs
        self.source_index = (np.concatenate([np.arange(lo, hi, dtype=np.int64) for lo, hi in segs]) if segs
                             else np.zeros(0, np.int64))
        self.n_available = self.total_frames = len(self.source_index)

    def resolve_segments(self) -> None:
        """``segments="court"``: scan [start, end), decide, set the segments (``run()`` does this before the first tracker)."""
        if not self._segments_pending:
            return
        from .. import activity as A
        opt = dict(self.segment_options)
        scan_kw = {k: opt.pop(k) for k in ("ref", "roi", "tau", "batch") if k in opt}
        opt.setdefault("fps", self.video_info.fps)
        t0 = timeit.default_timer()
        n = len(self.source_index)
        act = A.scan(self.video_path, engine=self.engine, start=self.start, end=self.start + n, **scan_kw)
        segs = [(self.start + lo, self.start + hi) for lo, hi in A.segments(A.court_view_mask(act, **opt))]
        self._segments_pending = False
        self._set_segments(segs)
        t1 = timeit.default_timer()
        self.timings["__segments__"] = {"seconds": t1 - t0, "frames": n, "kept": self.n_available, "segments": len(segs)}
        print(f"runner: court view in {self.n_available} of {n} frames, {len(segs)} segments ({n / max(t1 - t0, 1e-9):.1f} frames/s scanned)")

    def repair_identities(self) -> None:
        """``identities=True``: histograms of the stored player boxes over the kept frames, the assignment, and the ``Players``
        tracker's results replaced by relabelled ones (``run()`` does this between the trackers and ``draw_and_collect_data``)."""
        if not self.identities:
            return
        from .. import identity as I
        tracker = O.tracker_of(self.trackers.values(), "Players")      # the last one, as the projection takes it
        if tracker is None:
            print("runner: identities=True, but no tracker gives Players: nothing to relabel")
            return
        opt = dict(self.identity_options)
        scan_kw = {k: opt.pop(k) for k in ("every", "batch", "on_device") if k in opt}
        t0 = timeit.default_timer()
        results = tracker.results.predictions
        tracks = I.scan(self.video_path, results, engine=self.engine, positions=self.source_index[:len(results)], **scan_kw)
        self.identity_map, self.identity_distances = I.assign(tracks, **opt)
        tracker.results.predictions = [I.relabel(p, self.identity_map) for p in results]
        t1 = timeit.default_timer()
        n_players = int(opt.get("n_players", 4))
        assigned = sum(1 for v in self.identity_map.values() if v <= n_players)
        self.timings["__identities__"] = {"seconds": t1 - t0, "frames": len(results), "boxes": sum(t.boxes for t in tracks.values()),
                                          "tracks": len(tracks), "assigned": assigned, "unassigned": len(tracks) - assigned}
        print(f"runner: identities: {len(tracks)} tracks over {len(results)} frames -> {assigned} assigned, {len(tracks) - assigned} unassigned "
              f"({len(results) / max(t1 - t0, 1e-9):.1f} frames/s scanned)")

    def _pieces(self, lo: int = 0, hi: Optional[int] = None):
        """(kept position, source frame, count) of the parts of kept positions [lo, hi) that lie in one segment each."""
        hi = self.n_available if hi is None else min(hi, self.n_available)
        k = 0
        for slo, shi in self.segments:
            a, b = max(lo, k), min(hi, k + shi - slo)
            if a < b:
                yield a, slo + (a - k), b - a
            k += shi - slo

    def _batches(self, bs: int, lo: int = 0, hi: Optional[int] = None):
        """Lists of at most ``bs`` frames of kept positions [lo, hi), in order; with segments none spans a cut."""
        if self.segments is None:
            yield from _sampler(self._frames(lo, hi), bs)
            return
        for _, src, n in self._pieces(lo, hi):
            yield from _sampler(self._source_frames(src, src + n), bs)

    def _source_frames(self, lo: int, hi: int):
        return video.get_video_frames_generator(self.video_path, start=lo, stride=self.stride, end=hi)

    # ------------------------------------------------------------------ the output step (outputs.py)
    #: frames per Engine.render call / download / write of the output step
    RENDER_BATCH = 64

    @property
    def _projected(self) -> list:
        """``FrameProjection`` of frames [0, len): filled in frame order, the homography carrying over."""
        return self._outputs.proj.frames

    def restart(self) -> None:
        for tracker in self.trackers.values():
            tracker.restart()
        self._outputs.proj.restart()

    def draw_and_collect_data(self) -> None:
        self._outputs.draw_and_collect_data()

    def render_size(self) -> tuple:
        """(width, height) of the rendered clip: the source's, divided by ``render_scale``."""
        return self.video_info.width // self.render_scale, self.video_info.height // self.render_scale

    def frame_marks(self, i: int) -> list:
        """The marks of frame ``i`` of the annotated clip (``OutputStep.frame_marks``)."""
        return self._outputs.frame_marks(i)

    def inset_marks(self, i: int) -> list:
        return self._outputs.inset_marks(i)

    def trail_marks(self, results, i: int) -> list:
        return self._outputs.trail_marks(results, i)

    def topdown_marks(self, i: int) -> list:
        return self._outputs.topdown_marks(i)

    def _segment_start(self, i: int) -> int:
        """The first kept position of the segment that kept position ``i`` lies in (0 without segments)."""
        k = 0
        for lo, hi in self.segments or ():
            if i < k + hi - lo:
                return k
            k += hi - lo
        return 0 if self.segments is None else k

    def _frames(self, lo: int = 0, hi: Optional[int] = None):
        """Frames [start + lo, start + hi) of the clip (hi None: to self.end); with segments: kept positions [lo, hi)."""
        if self.segments is not None:
            return (f for _, src, n in self._pieces(lo, hi) for f in self._source_frames(src, src + n))
        end = self.end if hi is None else self.start + hi
        return video.get_video_frames_generator(self.video_path, start=self.start + lo, stride=self.stride, end=end)

    def run(self) -> None:
        self.resolve_segments()
        print(f"runner: Running {self.total_frames} frames")
        try:
            if self.fanout:
                self._run_fanout()
            else:
                for tracker in self.trackers.values():
                    # results (and the prediction caches) live on rank 0 only: its decision to skip a tracker is the one
                    # every rank follows, or the others would wait in the sharded path's collectives for ever
                    stored = D.broadcast_flag(len(tracker) != 0) if self.distributed else len(tracker) != 0
                    if stored:
                        print(f"{tracker.__str__()}: {len(tracker)} predictions stored")
                        continue
                    tracker.to(tracker.DEVICE)
                    print(f"{str(tracker)}: Running on {tracker.DEVICE} ...")
                    # registered before its loop and before anything is joined: neither an earlier tracker's error nor its own
                    # leaves what this tracker has queued uncollected
                    mine = _Deferred(tracker, t0=timeit.default_timer())
                    self._deferred.append(mine)
                    if self.distributed:
                        self._predict_sharded(tracker, mine)
                    else:
                        tracker.host_queue_depth = max(1, int(self.host_queue_depth))
                        tail: list = []
                        self._predict(tracker, defer=tail)
                        mine.wait = tail[0] if tail else None
                    mine.t1 = timeit.default_timer()
                    tracker.to("cpu")
                    # the trackers before this one had this tracker's whole device loop to finish their queued host stages
                    for d in self._deferred:
                        d.overlapped = d is not mine
                    self._join(merges=False, alone=False)
        finally:
            #  a tracker that raises must not leave finished work unsaved or a worker pool alive; a deferred stage's
            # own exception surfaces here, after the ones before it were saved
            self._join()
        self.repair_identities()
        self.draw_and_collect_data()

    def _predict(self, tracker: Tracker, defer: Optional[list] = None) -> None:
        """One tracker over the whole clip.  A stream tracker on the fp16 or the h2 arithmetic whose activations left the fp16
        range has switched itself one step up the ladder f16 -> default -> bx3 and asks to be run again (engine.RangeOverflow):
        at most twice; batch trackers repeat the offending batch themselves (yolo.YOLO.infer_frames).
        ``defer``: Tracker.predict_and_update."""
        from .. import engine as E

        def once():
            if self.segments is not None:
                self._predict_segments(tracker)
            else:
                tracker.predict_and_update(self._frames(), defer=defer, total_frames=self.total_frames)

        for _ in range(2):
            try:
                return once()
            except E.RangeOverflow as ex:
                print(f"{str(tracker)}: {ex}")
                tracker.restart()
                tracker.to(tracker.DEVICE)
        once()

    def _predict_segments(self, tracker: Tracker) -> None:
        """One tracker over the kept frames, segment by segment.  A batch tracker's loop (``Tracker._predict_batches``) runs once per
        segment and appends to its results: what it keeps between batches (ByteTrack) carries over, its batches end at the cut.  A
        stream tracker runs ``predict_partial`` + ``merge_partials`` per segment — its windows and sequences never span a cut — with
        the background set beforehand; results that carry a ``frame`` number get the kept position."""
        if self._is_batch_tracker(tracker):
            for _, src, n in self._pieces():
                tracker._predict_batches(self._source_frames(src, src + n), tracker.results.update, total_frames=n)
        else:
            self._segment_background(tracker)
            out: list = []
            for kept, src, n in self._pieces():
                part = tracker.merge_partials(tracker.predict_partial(self._source_frames(src, src + n), first_frame=kept, total_frames=n))
                assert len(part) == n, (str(tracker), len(part), n)
                for obj in part:
                    if kept and isinstance(getattr(obj, "frame", None), int):
                        obj.frame += kept
                out += part
            tracker.results.predictions = out
        print(f"{tracker.__str__()}: {len(tracker.results)} predictions.")

    def _segment_background(self, tracker) -> None:
        """A stream tracker's background (TrackNet's median), once, over the first ``min(median_max_sample_num, kept)`` kept frames —
        as ``_share_background`` computes it over the head of the clip."""
        if getattr(tracker, "median", None) is not None or not hasattr(tracker, "compute_median"):
            return
        nmed = min(tracker.median_max_sample_num, self.n_available)
        if nmed < 1:
            return
        frames = list(self._frames(0, nmed))
        if len(list(self._pieces(0, nmed))) > 1:       # kept frames of several segments are no contiguous range of a device clip
            frames = [video.host_frame(f) for f in frames]
        tracker.median = tracker.compute_median(frames)

    def _join(self, merges: bool = True, alone: bool = True) -> None:
        """Wait for deferred work, report and save (rank 0), in tracker order, host tails before merges.  ``merges`` False:
        only host tails; ``alone`` False: only those that had another tracker's loop to drain beside (or have nothing
        outstanding).  Every entry is collected even when one raises (the ones behind it are finished work too); the first error
        is raised afterwards.  With ``merges`` the merge thread ends.

        ``timings``: "seconds" is the tracker's own loop (sharded: device stage + gather).  "host_tail_seconds" is what was left
        to wait for of its queued host stages — after the next tracker's loop ("host_tail_overlapped"), normally nothing; a tail
        that drained with no loop beside it is part of "seconds".  "merge_seconds" is the merge's own span, which ran BESIDE the
        next tracker's shard ("merge_overlapped") — the two are not added: the next tracker's "seconds" already covers that wall
        time (no double counting)."""
        take = [d for d in self._deferred if (merges or not d.merge) and (alone or d.overlapped or d.wait is None)]
        self._deferred = [d for d in self._deferred if d not in take]
        first_error = None
        try:
            for d in sorted(take, key=lambda d: d.merge):
                ts = timeit.default_timer()
                try:
                    span = d.wait() if d.wait is not None else None
                except BaseException as exc:
                    first_error = first_error or exc
                    continue
                waited = timeit.default_timer() - ts
                if d.t1 is None:                    # its loop did not end: nothing to report
                    continue
                if d.merge:
                    self._report(d.tracker, d.t0, d.t1)
                    self.timings[str(d.tracker)].update(merge_seconds=span[1] - span[0], merge_overlapped=True)
                elif d.wait is None or d.overlapped:
                    self._report(d.tracker, d.t0, d.t1)
                    if d.wait is not None:
                        self.timings[str(d.tracker)].update(host_tail_seconds=waited, host_tail_overlapped=True)
                else:                               # a tail that drained with nothing beside it
                    self._report(d.tracker, d.t0, d.t1 + waited)
                    self.timings[str(d.tracker)].update(host_tail_seconds=waited)
                if not self.distributed or D.rank() == 0:
                    d.tracker.save_predictions()
        finally:
            if merges and self._merge_pool is not None:
                self._merge_pool.shutdown()
                self._merge_pool = None
        if first_error is not None:
            raise first_error

    def _report(self, tracker, t0, t1) -> None:
        print(f"{str(tracker)}: {t1 - t0} inference time.")
        n = len(tracker)
        self.timings[str(tracker)] = {"seconds": t1 - t0, "frames": n}
        if t1 > t0:
            print(f"{str(tracker)}: {n / (t1 - t0):.1f} frames/s")

    # ------------------------------------------------------------------ sharded over GPUs
    def _predict_sharded(self, tracker: Tracker, mine: _Deferred) -> None:
        """``mine``: the tracker's entry in ``run()``'s deferred list — a merge that goes to the merge thread is noted there."""
        rank, world = D.rank(), D.world_size()
        n = self.n_available
        lo, hi = D.shard_range(n, rank, world)
        ch, ct = tracker.temporal_context
        head, tail = min(ch, lo), min(ct, n - hi)
        if ch or ct:
            self._share_background(tracker)
        from .. import engine as E

        def attempt():
            if hi <= lo:
                return [], False
            try:
                return tracker.predict_partial(self._frames(lo - head, hi + tail), first_frame=lo, head_context=head,
                                               tail_context=tail, total_frames=hi - lo), False
            except E.RangeOverflow as ex:                  # a stream tracker switched itself to the full-range kernels
                print(f"{str(tracker)}: {ex}")
                return None, True

        # where the tracker stands on the ladder f16 -> default (h2) -> bx3; a tracker without the switch counts as at its end
        def level():
            return {"f16": 0, "h2": 1}.get(getattr(tracker, "arithmetic", None), 2)

        was_full, was = tracker.full_range, level()
        partial, over = attempt()
        # A step of the ladder is decided for ALL ranks at once: a rank whose shard overflowed (stream trackers raise, batch
        # trackers switch inside the offending batch) must not leave the others waiting in the gather, and the merged result
        # must come from one arithmetic.  Every rank enters these collectives; the ranks then stand where the furthest one
        # stands (use_full_range is not called on a rank already there) and repeat.  At most twice: f16 -> default, default -> bx3
        for _ in range(2):
            if not D.any_flag(over or level() != was or (not was_full and tracker.full_range)):
                break
            target = 2 if D.any_flag(level() >= 2) else 1 if D.any_flag(level() >= 1) else 0
            print(f"{str(tracker)}: activations left the fp16 range on some rank — every rank repeats its shard on the "
                  f"{'bf16x3' if target == 2 else 'default fp32-equivalent'} path")
            for _step in range(2):
                if level() < target:
                    tracker.use_full_range()
            tracker.to(tracker.DEVICE)
            was_full, was = tracker.full_range, level()
            partial, over = attempt()
        assert not over
        assert len(partial) == hi - lo, (str(tracker), len(partial), lo, hi)
        # the partials travel as arrays (counts + rows per rank: two collectives, O(bytes)); trackers whose partials are not
        # arrays fall back to one pickled buffer per rank.  Every rank must take the same branch: agreed by a collective
        packed = tracker.pack_partials(partial)
        if not D.any_flag(packed is None):
            parts = D.gather_arrays(packed, dst=0)
            allp = None if parts is None else [x for a in parts for x in tracker.unpack_partials(a)]
        else:
            allp = D.gather_results(partial, dst=0)
        if rank == 0:
            def merge():
                ts = timeit.default_timer()
                with relaxed_gc():
                    tracker.results.predictions = tracker.merge_partials(allp)
                print(f"{tracker.__str__()}: {len(tracker.results)} predictions.")
                return ts, timeit.default_timer()
            # The sequential stage (ByteTrack ids over ALL frames in global order: ~60 us per frame of host C++) is rank 0's
            # alone.  Where it touches no GPU it runs on a worker thread while rank 0's GPU starts on the next tracker's shard —
            # otherwise the other ranks would wait for it at the next gather; run() joins before it returns
            if tracker.merge_is_host_only and world > 1:
                if self._merge_pool is None:
                    self._merge_pool = ThreadPoolExecutor(max_workers=1)
                mine.wait, mine.merge = self._merge_pool.submit(merge).result, True
            else:
                merge()

    def _share_background(self, tracker) -> None:
        """TrackNet's background median (iterable.py:59-81) is a property of the clip's first frames: rank 0
        computes it (on its GPU), every rank receives the (h, w, 3) uint8 array."""
        if getattr(tracker, "median", None) is not None or not hasattr(tracker, "compute_median"):
            return
        med = None
        if D.rank() == 0:
            nmed = min(tracker.median_max_sample_num, self.n_available)
            med = tracker.compute_median(list(self._frames(0, nmed)))
        tracker.median = D.broadcast_array(med, (self.video_info.height, self.video_info.width, 3), np.uint8, src=0)

    # ------------------------------------------------------------------ one decode / one upload for all trackers
    def _run_fanout(self) -> None:
        todo = [t for t in self.trackers.values() if len(t) == 0]
        for t in self.trackers.values():
            if len(t) != 0:
                print(f"{t.__str__()}: {len(t)} predictions stored")
        if not todo:
            return
        batch = [t for t in todo if self._is_batch_tracker(t)]
        stream = [t for t in todo if t not in batch]
        bs = max([t.batch_size for t in batch] or [max(t.batch_size for t in stream)])
        for t in todo:
            t.to(t.DEVICE)
            print(f"{str(t)}: Running on {t.DEVICE} (fan-out, {bs} frames per upload) ...")
        t0 = timeit.default_timer()

        # the host stages of all batch trackers share one queue (no copies: the device stages hand out their own arrays here) and
        # trail the device stages by one stage per tracker; a tracker without stages is updated in line
        # (the staging of host frames is the walk's: freed after the queue has drained, whatever ends the pass)
        with video.ResidentBatches(self.engine, _sampler(self._frames(), bs), bs, self.video_info.resolution_wh[::-1], prefetch=True) as walk, \
                host_stages(len(batch)) as queue:
            for sample, _ in walk:
                for t in batch:
                    for sub in _sampler(iter(sample), t.batch_size):
                        if t._has_stages():
                            queue.put(t.post_sample, t.infer_sample(sub), t.results.update)
                        else:
                            t.results.update(t.predict_sample(sub))
            queue.finish()
        # stream trackers (TrackNet needs the clip's background median before its first window): their own pass —
        # over the same HBM-resident handles when the clip lives in HBM, else a second read of the source
        for t in stream:
            self._predict(t)
        t1 = timeit.default_timer()
        for t in todo:
            t.to("cpu")
            print(f"{t.__str__()}: {len(t.results)} predictions.")
            t.save_predictions()       # (the trackers share every upload: only the combined time below is meaningful)
        self.timings["__fanout__"] = {"seconds": t1 - t0, "frames": self.total_frames}
        print(f"runner: fan-out pass {t1 - t0} inference time, {self.total_frames / max(t1 - t0, 1e-9):.1f} frames/s (all trackers)")

    @staticmethod
    def _is_batch_tracker(t: Tracker) -> bool:
        """Batch trackers answer predict_frames with NoPredictFrames (reference tracker.py:315-326)."""
        if getattr(t, "streams", None) is not None:
            return not t.streams
        try:
            t.predict_frames(iter(()))
        except NoPredictFrames:
            return True
        except Exception:
            return False
        return False
