"""Worker of tests/test_f16_range_guard_host.py (one process per rank, gloo): the sharded runner's decision on the range ladder
f16 -> default (h2) -> bx3, over the fakes of tests/dist_worker.py with the ``half`` switch added.  Modes:
  ladder — every tracker starts with ``half=True``.  In the first attempt rank 1's models leave the fp16 range (the batch tracker's
           model switches f16 -> default inside its second batch, the stream tracker raises engine.RangeOverflow): both ranks repeat on
           the default path.  In that second attempt rank 0's models overflow on h2: both ranks repeat on bx3.  Three attempts
           per tracker and rank, no assert of the runner fires, every rank ends on bx3;
  bx3    — the same trackers on bx3 from the first frame (world 1): what the merged predictions of "ladder" must equal.
The arithmetic is visible in the fake numbers (a shift per arithmetic), so a result merged from two of them could not pass.
Usage: python tests/range_guard_worker.py MODE RANK WORLD PORT OUT"""
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tests import dist_worker as W  # noqa: E402  (registers the synthetic:// frame source)

OVERFLOWS = {}            # arithmetic -> the rank whose models leave the fp16 range on it ("ladder": {"f16": 1, "h2": 0})
SHIFT = {"f16": 0.5, "h2": 0.0, "bx3": 0.25}


class LadderYOLO(W.FakeYOLO):
    """FakeYOLO with yolo.YOLO's two switches; like ``YOLO.infer_frames`` it takes one step inside the offending batch."""

    def __init__(self, model_path, engine=None, half=False):
        super().__init__(model_path, engine, half)
        self.half, self.fp32_mode, self.fell_back, self.batches = bool(half), "h2", False, 0

    @property
    def arithmetic(self):
        return "f16" if self.half else self.fp32_mode

    def set_half(self, half):
        self.half, self.batches = bool(half), 0

    def set_fp32_mode(self, mode):
        self.fp32_mode, self.batches = mode, 0

    def _shift(self):
        self.batches += 1
        if self.batches == 2 and OVERFLOWS.get(self.arithmetic) == W.MY_RANK:
            if self.half:
                self.set_half(False)
            else:
                self.set_fp32_mode("bx3")
            self.fell_back = True
        return SHIFT[self.arithmetic]


def _arith(graph):
    from padel_analytics_amd import graph as G
    return {G.DTYPE_F16: "f16", G.DTYPE_H2: "h2"}.get(graph.dtype, "bx3")


class LadderModel(W.FakeModel):
    raised = set()        # arithmetics this process's TrackNet has overflowed on already (once each)

    def take_overflow(self):
        a = _arith(self.graph)
        if OVERFLOWS.get(a) == W.MY_RANK and a not in LadderModel.raised:
            LadderModel.raised.add(a)
            return True
        return False


class LadderSession(W.FakeBallSession):
    def __init__(self, model, h, w):
        super().__init__(model, h, w)
        self.shift = {"f16": 0.031, "h2": 0.0, "bx3": 0.013}[_arith(model.graph)]


def run(mode, rank, world, out):
    from oracle import tracknet_ref as tr
    from padel_analytics_amd import checkpoint, detections as D, engine as E, yolo
    from padel_analytics_amd.trackers import BallTracker, PlayerTracker, TrackingRunner
    from padel_analytics_amd.trackers import players_tracker
    W.MY_RANK = rank
    for mod in (players_tracker, yolo):
        mod.YOLO = LadderYOLO
    E.Model, E.BallSession = LadderModel, LadderSession
    E.default_engine = lambda *a, **k: None
    assert E.fp32_mode() == "h2", "the ladder's middle step is the default arithmetic"
    tmp = Path(tempfile.mkdtemp())
    checkpoint.save_checkpoint(tmp / "tracknet.pt", tr.synth_tracknet_state_dict(9), "tracknet", param_dict={"seq_len": 8, "bg_mode": "concat"})
    zone = D.PolygonZone(np.array([[10, 10], [118, 10], [118, 66], [10, 66]]), frame_resolution_wh=(128, 72))
    half = mode == "ladder"
    trackers = [PlayerTracker("players.pt", zone, batch_size=8, half=half),
                BallTracker(str(tmp / "tracknet.pt"), None, batch_size=8, median_max_sample_num=20, half=half)]
    attempts = {}
    for t in trackers:
        if mode == "ladder":
            assert t.arithmetic == "f16" and t.full_range
        else:
            for _ in range(2):
                t.use_full_range()
            assert t.arithmetic == "bx3"
        orig = t.predict_partial
        attempts[str(t)] = []
        t.predict_partial = lambda *a, _o=orig, _t=t, **k: (attempts[str(_t)].append(_t.arithmetic), _o(*a, **k))[1]
    if mode == "ladder":
        OVERFLOWS.update({"f16": 1, "h2": 0})
    TrackingRunner(trackers, "synthetic://?n=45&h=72&w=128&fps=30&seed=3", tmp / "out.mp4", distributed=world > 1).run()
    for t in trackers:
        assert t.arithmetic == "bx3" and not getattr(t, "half", False), (str(t), t.arithmetic)
        if mode == "ladder":
            assert attempts[str(t)] == ["f16", "h2", "bx3"], (rank, str(t), attempts[str(t)])
    if rank == 0:
        Path(out).write_text(json.dumps({str(t): [o.serialize() for o in t.results.predictions] for t in trackers}))


def main():
    mode, rank, world, port, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    if world > 1:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
        dist.init_process_group("gloo", rank=rank, world_size=world)
    run(mode, rank, world, out)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
