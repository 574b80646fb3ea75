"""The output step of ``TrackingRunner`` (``draw_and_collect_data``, reference ``trackers/runner.py`` :91-173): what is made of the
trackers' stored results once they have run.  The runner's docstring is the manual of the keyword arguments; this is how the step works.

* ``tracker_of`` / ``results_of`` are the one lookup "the tracker whose ``object()`` is X, the last one if several" (reference :141-146).
* ``Projections`` holds the ``FrameProjection`` of every kept frame — the homography is a state machine over the frames, so they are
  filled in frame order and kept — and puts the players' positions into ``DataAnalytics``.
* One class per output, each with the same few methods (``Output``): the constructor checks — in ``TrackingRunner.__init__``, before
  any tracker runs, before a file exists —, ``open`` creates the sink and the buffers, ``batch`` does one batch, ``finish`` ends a walk
  that came through, ``close`` frees and closes whatever ended it, ``report`` writes the ``timings`` entry and the printed line.  Each
  owns its buffers, its sink and its clock.  ``AnnotatedClip`` (``render=``): one ``Engine.render`` to YUV 4:2:0 in the sink's geometry,
  one download, one write.  ``TopDownClip`` (``topdown=``): one ``Engine.warp`` of the batch into a BGR canvas buffer, with ``heatmap=``
  one ``Engine.heat`` on it, one ``Engine.render`` of that buffer with the canvas marks into the second sink's geometry, one download,
  one write.  ``HeatMaps`` (``heatmap=``): with a canvas the maps live in HBM for the walk and the top-down clip drives them; without
  one they are accumulated on the host from the stored results alone.
* ``OutputStep.walk`` is the ONE loop over batches of ``TrackingRunner.RENDER_BATCH`` frames: BGR in HBM (``video.ResidentBatches``)
  when an output needs frames, plain ranges of kept positions when none does — no frame is read then, no GPU touched.  Each batch is
  projected (and, with the inset or the collection on, collected) first, then handed to every output in the order annotated clip,
  top-down clip, heat maps."""
from __future__ import annotations

import contextlib
import os
import timeit
from typing import Optional

from .. import dist as D, video


def object_name(tracker) -> Optional[str]:
    """The name of the tracker's result type (``Players`` / ``Ball`` / ``Keypoints`` are what the projection looks for); None
    for a holder of results that states none."""
    obj = getattr(tracker, "object", None)
    return getattr(obj(), "__name__", None) if callable(obj) else None


def tracker_of(trackers, name: str):
    """The tracker among ``trackers`` whose result type is ``name`` — the last one, if several (reference :141-146) — or None."""
    found = None
    for tracker in trackers:
        if object_name(tracker) == name:
            found = tracker
    return found


def results_of(trackers, name: str, lo: int, n: int) -> list:
    """The stored results of frames [lo, lo + n) of ``tracker_of(trackers, name)``: None where it has none, or there is no such tracker."""
    tracker = tracker_of(trackers, name)
    return [tracker.results[i] if tracker is not None and i < len(tracker.results) else None for i in range(lo, lo + n)]


class Projections:
    """``frames``: the ``FrameProjection`` of kept frames [0, len), computed once from the results stored at that moment and kept until
    ``restart``.  ``collect`` also fills the runner's ``data_analytics``; ``seconds`` is the host time of both."""

    def __init__(self, run) -> None:
        self.run = run
        self.frames: list = []
        self.seconds = 0.0
        self._told: set = set()            # what was said once about missing data

    def restart(self) -> None:
        """Forget the projections and what was collected: the homography is a state machine over the frames from the first one on."""
        if self.run.data_analytics is not None:    # (not its truth value: that is len(), 0 after a clip of no frames)
            self.run.data_analytics.restart()
        self.frames, self.run.projected_court.H, self.seconds = [], None, 0.0

    def _tell_once(self, what: str) -> None:
        if what not in self._told:
            self._told.add(what)
            print(f"runner: {what}")

    def through(self, hi: int) -> None:
        """Projections of frames [len(self.frames), hi), ``RENDER_BATCH`` at a time, in frame order: each frame's Players / Ball /
        Keypoints are the stored results of the tracker of that type."""
        run = self.run
        t0 = timeit.default_timer()
        while len(self.frames) < hi:
            lo = len(self.frames)
            n = min(run.RENDER_BATCH, hi - lo)
            per = [results_of(run.trackers.values(), name, lo, n) for name in ("Keypoints", "Players", "Ball")]
            self.frames += run.projected_court.project_batch(*per, run.is_fixed_keypoints)
        self.seconds += timeit.default_timer() - t0

    def collect(self, lo: int, n: int) -> None:
        """Frames [lo, lo + n): project them, and put every projected player's position, in metres from the court centre, into
        ``data_analytics`` (reference :541-567), one ``step`` per frame (:159-160).  Where the reference prints, frame after frame,
        that data are missing, this says so once."""
        self.through(lo + n)
        t0 = timeit.default_timer()
        data = self.run.data_analytics
        shift = self.run.projected_court.court_keypoints.shift_point_origin
        for fp in self.frames[lo:lo + n]:
            if fp.H is None:
                self._tell_once("no homography for some frames (no court keypoints): nothing is projected there")
            elif fp.players is None:
                self._tell_once("Missing data for players projection in some frames")
            if data is not None:
                for player in fp.players or ():
                    data.add_player_position(id=player.id, position=shift(tuple(float(v) for v in player.projection), "meters"))
                data.step(1)
        self.seconds += timeit.default_timer() - t0


class Output:
    """One output of the step.  ``sink`` / ``own``: where its frames go and whether the step closes it; ``buffers``: what ``close`` frees."""
    needs_frames = True
    sink, own, buffers = None, False, ()

    def __init__(self, step: "OutputStep") -> None:
        self.step, self.run = step, step.run

    def open(self, eng, batch: int) -> None:
        """The sink and the buffers of a walk in batches of at most ``batch`` frames."""

    def batch(self, src, lo: int, n: int) -> None:
        """Kept frames [lo, lo + n); ``src``: their BGR in HBM (None in a walk that reads no frame)."""

    def finish(self) -> None:
        """The walk came through: what the output makes of the whole clip."""

    def close(self) -> None:
        """Safe after an ``open`` that failed: what was allocated by then is freed, a sink opened by then is closed."""
        for buf in self.buffers:
            buf.free()
        self.buffers = ()
        if self.own:
            self.sink.close()

    def report(self, done: int) -> None:
        pass

    def _open_sink(self, eng, target, w: int, h: int) -> None:
        self.eng, self.buffers, self.sink, self.own = eng, [], None, False
        self.sink, self.own = video.open_sink(target, w, h, self.run.video_info.fps, self.run.render_quality)

    def _alloc(self, nbytes: int):
        self.buffers.append(self.eng.alloc(nbytes))
        return self.buffers[-1]

    def _written(self):
        b = getattr(self.sink, "bytes_written", None)
        return os.path.getsize(self.sink.path) if b is None and self.own else b


class AnnotatedClip(Output):
    """``render=``: the clip with every tracker's results drawn on it (``OutputStep.frame_marks``), at 1 / ``render_scale`` of its size."""

    def __init__(self, step) -> None:
        """``ValueError`` for a ``render_scale`` this clip's size does not allow — the rendered frames are YUV 4:2:0: the source must
        be a multiple of the scale each way and the output even — naming the scales that would work, and for a caller's
        ``FrameSink`` of another size than the rendered frames.  (A path the sink refuses is refused when it is opened.)"""
        super().__init__(step)
        run = self.run
        w, h, s = run.video_info.width, run.video_info.height, run.render_scale
        fits = [k for k in (1, 2, 3, 4) if w % k == 0 and h % k == 0 and (w // k) % 2 == 0 and (h // k) % 2 == 0 and w // k >= 2 and h // k >= 2]
        if s != 1 and s not in fits:
            raise ValueError(f"render_scale={s}: the {w} x {h} clip does not divide into even {s} x {s}-averaged frames "
                             f"(render_scale that works for this clip: {', '.join(str(k) for k in fits) or 'none'})")
        if isinstance(run.render, video.FrameSink):
            wo, ho = run.render_size()
            try:
                video.check_sink(run.render, wo, ho)
            except ValueError as exc:
                raise ValueError(f"render: {exc}, the {w} x {h} clip at render_scale={s} gives {wo} x {ho}") from None

    def open(self, eng, batch: int) -> None:
        wo, ho = self.run.render_size()
        self._open_sink(eng, self.run.render, wo, ho)
        print(f"runner: Writing results into {getattr(self.sink, 'path', self.sink)}")
        self.dst = self._alloc(video.yuv_span(batch, ho, wo, self.sink.desc))
        self.step.t0 = timeit.default_timer()          # the walk's clock starts behind the clip's own sink

    def batch(self, src, lo: int, n: int) -> None:
        from .. import engine as E, render as R
        run, sink = self.run, self.sink
        w, h = run.video_info.width, run.video_info.height
        wo, ho = run.render_size()
        # (only a scale other than 1 is passed on: an engine that has never heard of the argument still renders at full size)
        scaled = {"scale": run.render_scale} if run.render_scale != 1 else {}
        marks, first = R.pack([self.step.frame_marks(lo + k) for k in range(n)])
        self.eng.render(src, n, h, w, marks, first, self.dst, out=E.RENDER_YUV420, geom=sink.desc, enc=sink.enc, **scaled)
        sink.write_device(self.dst.view(0, video.yuv_span(n, ho, wo, sink.desc)), n)

    def report(self, done: int) -> None:
        step = self.step
        # (with topdown= as well: the walk without the top-down view's own steps)
        seconds = step.t1 - step.t0 - (step.top.seconds if step.top is not None else 0.0)
        self.run.timings["__render__"] = {"seconds": seconds, "frames": done, "bytes": self._written()}
        print(f"runner: rendered {done} frames in {seconds:.3f} s ({done / max(seconds, 1e-9):.1f} frames/s: render + download + write)")


class TopDownClip(Output):
    """``topdown=``: every frame warped through its court homography into the canvas ``view``, the canvas marks on it
    (``OutputStep.topdown_marks``).  With ``heatmap=`` the maps live in HBM beside the canvases (``heat_dev``), zero at the start of the
    walk, and every batch gets one ``Engine.heat`` between the warp and the canvas render."""

    def __init__(self, step, trackers, options: dict) -> None:
        """The canvas, and a ``ValueError`` for a run that could not write the clip: no tracker gives ``Keypoints`` (no homography,
        ever), ``fanout``, a canvas the sink refuses, a caller's ``FrameSink`` of another size than the canvas."""
        from .. import topdown as T
        super().__init__(step)
        run = self.run
        if run.fanout:
            raise ValueError("topdown= is not available with fanout=True")
        if tracker_of(trackers, "Keypoints") is None:
            raise ValueError("topdown=: no tracker gives Keypoints, so no frame would have a court homography to be warped through")
        self.view = T.TopDownView(run.projected_court, **options)
        self.seconds, self.heat_dev = 0.0, None
        w, h = self.view.size
        try:
            video.check_sink(run.topdown, w, h, run.render_quality)
        except ValueError as exc:
            if isinstance(run.topdown, video.FrameSink):
                raise ValueError(f"topdown: {exc}, the canvas is {w} x {h}") from None
            raise ValueError(f"topdown: the {w} x {h} canvas cannot be written to {run.topdown}: {exc}") from None

    def open(self, eng, batch: int) -> None:
        ts = timeit.default_timer()
        view, heat_state = self.view, self.run.heat_state
        self.seconds, self.heat_dev = 0.0, None
        self._open_sink(eng, self.run.topdown, *view.size)
        print(f"runner: Writing the top-down view into {getattr(self.sink, 'path', self.sink)}")
        self.canvas = self._alloc(batch * view.h * view.w * 3)
        self.dst = self._alloc(video.yuv_span(batch, view.h, view.w, self.sink.desc))
        if self.step.maps is not None:
            self.heat_dev = self._alloc(heat_state.nbytes).upload(heat_state)
        self.seconds += timeit.default_timer() - ts

    def batch(self, src, lo: int, n: int) -> None:
        from .. import engine as E, render as R
        ts = timeit.default_timer()
        run, view, sink, eng = self.run, self.view, self.sink, self.eng
        matrices, valid = view.matrices(self.step.proj.frames[lo:lo + n])
        eng.warp(src, n, run.video_info.height, run.video_info.width, matrices, valid, self.canvas, view.h, view.w, fill=view.fill)
        if self.heat_dev is not None:
            self.step.maps.on_canvas(eng, self.canvas, self.heat_dev, lo, n)
        marks, first = R.pack([self.step.topdown_marks(lo + k) for k in range(n)])
        eng.render(self.canvas, n, view.h, view.w, marks, first, self.dst, out=E.RENDER_YUV420, geom=sink.desc, enc=sink.enc)
        sink.write_device(self.dst.view(0, video.yuv_span(n, view.h, view.w, sink.desc)), n)
        self.seconds += timeit.default_timer() - ts

    def report(self, done: int) -> None:
        step, view = self.step, self.view
        # alone: the whole walk; beside render=: its own steps (matrices and marks, warp, render, download / encode, write)
        seconds = self.seconds if step.clip is not None else step.t1 - step.t0
        self.run.timings["__topdown__"] = {"seconds": seconds, "frames": done, "bytes": self._written()}
        print(f"runner: top-down view: {done} frames of {view.w} x {view.h} in {seconds:.3f} s ({done / max(seconds, 1e-9):.1f} frames/s: "
              f"warp + render + download + write)")


class HeatMaps(Output):
    """``heatmap=``: the runner's ``heat_state``, and the file made of it when the walk has come through (``HeatMap.save``).  Beside
    ``topdown=`` the top-down clip accumulates them on its canvases (``on_canvas``); without a canvas to show them on ``batch`` does, on
    the host, from the stored results alone.  ``seconds``: the heat calls, the download and the save."""
    needs_frames = False
    OPTIONS = ("radius_m", "saturate_s", "alpha", "ids", "show", "overlay")

    def __init__(self, step, trackers, options: dict, canvas_options: dict) -> None:
        """The maps' parameters, and a ``ValueError`` for a run that could not make them: ``fanout``, no tracker that gives
        ``Keypoints`` or none that gives ``Players``, a path that ends in neither ``.npy`` nor ``.jpg``, an option ``HeatMap`` does not
        know or refuses, a canvas the JPEG encoder refuses."""
        from .. import heatmap as HM, topdown as T
        super().__init__(step)
        run = self.run
        if run.fanout:
            raise ValueError("heatmap= is not available with fanout=True")
        for name in ("Keypoints", "Players"):
            if tracker_of(trackers, name) is None:
                raise ValueError(f"heatmap=: no tracker gives {name}, so no player would ever have a place on the court")
        suffix = os.path.splitext(str(run.heatmap))[1].lower()
        if suffix not in (".npy", ".jpg"):
            raise ValueError(f"heatmap={str(run.heatmap)!r}: the path must end in .npy (the maps) or .jpg (a picture of them)")
        unknown = sorted(set(options) - set(self.OPTIONS))
        if unknown:
            raise ValueError(f"heatmap_options: unknown {', '.join(unknown)} (known: {', '.join(self.OPTIONS)})")
        self.overlay = bool(options.pop("overlay", True))          # the top-down clip shows the maps
        view = step.top.view if step.top is not None else T.TopDownView(run.projected_court, **canvas_options)
        self.heat = HM.HeatMap(view, fps=run.video_info.fps, **options)
        self.seconds = 0.0
        if suffix == ".jpg":
            try:
                video.jpeg_desc(view.w, view.h, run.render_quality)
            except ValueError as exc:
                raise ValueError(f"heatmap: the {view.w} x {view.h} canvas cannot be written to {run.heatmap}: {exc}") from None

    def restart(self) -> None:
        """Every ``draw_and_collect_data`` starts from maps of zeros."""
        self.run.heat_state, self.seconds = self.heat.state(), 0.0

    def points(self, lo: int, n: int) -> tuple:
        """(points, first, valid) of kept frames [lo, lo + n) (``HeatMap.batch``): the frames' projections and the stored ``Players``."""
        self.step.proj.through(lo + n)
        return self.heat.batch(self.step.proj.frames[lo:lo + n], results_of(self.run.trackers.values(), "Players", lo, n))

    def on_canvas(self, eng, canvas, state_dev, lo: int, n: int) -> None:
        """Frames [lo, lo + n) into the maps in ``state_dev``, and the maps as they stand over the ``n`` canvases in ``canvas``."""
        t0 = timeit.default_timer()
        view = self.heat.view
        eng.heat(canvas, n, view.h, view.w, state_dev, self.heat.planes, *self.points(lo, n), **self.heat.call(self.overlay))
        self.seconds += timeit.default_timer() - t0

    def batch(self, src, lo: int, n: int) -> None:
        if self.step.top is not None:              # the top-down clip has put them on its canvases
            return
        from .. import heatmap as HM
        t0 = timeit.default_timer()
        HM.accumulate_host(None, self.run.heat_state, *self.points(lo, n), **self.heat.call(overlay=False))
        self.seconds += timeit.default_timer() - t0

    def finish(self) -> None:
        t0 = timeit.default_timer()
        run, top = self.run, self.step.top
        on_device = {}
        if top is not None:
            top.heat_dev.download(run.heat_state)
            on_device = dict(eng=top.eng, canvas=top.canvas, state_dev=top.heat_dev)
        self.heat.save(run.heatmap, run.heat_state, run.render_quality, **on_device)
        self.seconds += timeit.default_timer() - t0

    def report(self, done: int) -> None:
        heat = self.heat
        self.run.timings["__heatmap__"] = {"seconds": self.seconds, "frames": done}
        print(f"runner: heat maps of {done} frames ({heat.planes} of {heat.view.w} x {heat.view.h}) written to {self.run.heatmap} "
              f"in {self.seconds:.3f} s")


class OutputStep:
    """The outputs ``run`` (the ``TrackingRunner``) was asked for — its public attributes are read when the step runs —, the
    projections they share, and the walk.  ``t0`` / ``t1``: the walk's clock."""

    def __init__(self, run, trackers, topdown_options: Optional[dict], heatmap_options: Optional[dict]) -> None:
        self.run = run
        self.proj = Projections(run)
        self.t0 = self.t1 = 0.0
        self.clip = self.top = self.maps = None
        if run.render is not None:                 # now: a scale or a sink that does not fit the clip costs no tracker run
            self.clip = AnnotatedClip(self)
        if run.topdown is not None:
            self.top = TopDownClip(self, trackers, dict(topdown_options or {}))
        if run.heatmap is not None:
            self.maps = HeatMaps(self, trackers, dict(heatmap_options or {}), dict(topdown_options or {}))

    def draw_and_collect_data(self) -> None:
        run = self.run
        active = [out for out in (self.clip, self.top, self.maps) if out is not None]
        if not active and run.data_analytics is None:
            print("runner: drawing / data collection is outside the hot path of this build (skipped)")
            return
        if run.distributed and D.rank() != 0:      # the results live on rank 0
            return
        projecting = run.court_inset or run.data_analytics is not None
        # every pass starts over: a second call does not append the clip's datapoints again, and projections that frame_marks /
        # inset_marks cached before the trackers had stored their results do not stay
        self.proj.restart()
        if self.maps is not None:
            self.maps.restart()
        done = self.walk(active, projecting)
        for out in active:
            out.report(done)
        if run.data_analytics is not None:
            run.data_analytics.frames = run.data_analytics.frames[:-1]            # reference :167: remove the extra frame
            print(f"runner: collected the players' positions of {done} frames ({len(run.data_analytics)} in data_analytics)")
        if projecting:
            run.timings["__collect__"] = {"seconds": self.proj.seconds, "frames": done}

    def walk(self, active: list, collecting: bool) -> int:
        """The kept frames once, ``RENDER_BATCH`` at a time, through every output of ``active`` -> the number of frames.  Whatever ends
        it: synchronize, then close every output that was opened."""
        run = self.run
        bs, total = run.RENDER_BATCH, run.n_available
        eng = None
        if any(out.needs_frames for out in active):
            from .. import engine as E
            eng = run.engine or E.default_engine()
            batches = video.ResidentBatches(eng, run._batches(bs), bs, (run.video_info.height, run.video_info.width))
        else:                                      # the stored results alone: ranges of kept positions in the frames' place
            batches = contextlib.nullcontext((range(lo, min(lo + bs, total)), None) for lo in range(0, total, bs))
            collecting = True                      # (says once what is missing, as the collection does)
        opened, done = [], 0
        self.t0 = timeit.default_timer()
        try:
            for out in active:
                opened.append(out)
                out.open(eng, bs)
            with batches as walk:
                for frames, _ in walk:
                    n = len(frames)
                    if collecting:
                        self.proj.collect(done, n)
                    elif self.top is not None:
                        self.proj.through(done + n)
                    src = video.device_batch(frames)[0] if eng is not None else None
                    for out in active:
                        out.batch(src, done, n)
                    done += n
            for out in active:
                out.finish()
        finally:
            if eng is not None:
                eng.synchronize()
            for out in opened:
                out.close()
        self.t1 = timeit.default_timer()
        return done

    # ------------------------------------------------------------------ the marks
    def inset_marks(self, i: int) -> list:
        """The court inset of frame ``i``, in the reference's order (:630-668): the panel and the court, the projected players,
        the projected ball."""
        self.proj.through(i + 1)
        fp = self.proj.frames[i]
        marks = self.run.projected_court.inset_marks()
        if fp.players is not None:
            marks += fp.players.projection_marks()
        if fp.ball is not None:
            marks += fp.ball.projection_marks()
        return marks

    def trail_marks(self, results, i: int) -> list:
        """The ball's trail at kept position ``i`` (reference ``ball_tracker.py:299-347``, ``draw_multiple_frames`` / ``draw_traj``:
        a queue of the last positions, an invisible ball taking a place in it, each drawn as a white circle of radius 3 with a
        yellow outline): the positions of the ``ball_trail`` kept frames i, i - 1, ... that lie in i's segment and hold a visible
        ball, newest first, each a disc of radius 3 in RGB (255, 255, 0) under one of radius 2 in white."""
        from .. import render as R
        marks = []
        for j in range(min(i, len(results) - 1), max(self.run._segment_start(i), i - self.run.ball_trail + 1) - 1, -1):
            ball = results[j]
            if ball.visibility:
                x, y = ball.asint()
                marks += [R.disc(x, y, 3, (0, 255, 255)), R.disc(x, y, 2, (255, 255, 255))]
        return marks

    def frame_marks(self, i: int) -> list:
        """The marks of frame ``i`` (counted from ``start``; with segments: kept position ``i``, and the label shows the source frame,
        ``source_index[i] - start + 1``): ``FRAME: i + 1`` (reference :118-127, there cv2's Hershey font in RGB
        (255, 255, 0) with its bottom-left at (20, 50); here the renderer's font at scale 3), then every tracker's
        ``results[i].marks(**tracker.draw_kwargs())`` in tracker order (with ``ball_trail`` the ``Ball`` tracker's is followed by
        ``trail_marks``), then — with ``court_inset`` — ``inset_marks(i)``.  The
        projections behind the inset are computed once, in frame order, from the results stored at that moment and kept until the next
        ``draw_and_collect_data`` or ``restart``, which start over."""
        from .. import render as R
        run = self.run
        k = 3
        marks = R.text(f"FRAME: {int(run.source_index[i]) - run.start + 1 if i < len(run.source_index) else i + 1}", 20, 50 - (R.GLYPH_H * k - 1), k, (0, 255, 255))
        for tracker in run.trackers.values():
            if i < len(tracker.results):
                marks += tracker.results[i].marks(**tracker.draw_kwargs())
                if run.ball_trail > 0 and object_name(tracker) == "Ball":
                    marks += self.trail_marks(tracker.results, i)
        if run.court_inset:
            marks += self.inset_marks(i)
        return marks

    def topdown_marks(self, i: int) -> list:
        """The marks of canvas frame ``i`` (``TopDownView.marks``): the frame's projection, and the stored ``Players`` / ``Ball``."""
        self.proj.through(i + 1)
        trackers = self.run.trackers.values()
        return self.top.view.marks(self.proj.frames[i], results_of(trackers, "Players", i, 1)[0], results_of(trackers, "Ball", i, 1)[0])
