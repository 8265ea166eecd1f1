"""Device-resident driver of the hot path for frame streams and benchmarks.

torch is used for what it is good at here -- device buffers, the current HIP stream,
torch.distributed -- and nothing else: every computation goes through the C ABI
(capi.Context -> libpagk_hip.so).  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import capi, distributed


def _event_on(stream):
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev


class GatherRing:
    """The two alternating buffers of the sharded step's all-gather and the event ordering around them, apart from the
    streams so that the ordering can be tested without a GPU (tests/test_distributed_cpu.py).  The result of step k stays
    intact while step k+1's gather runs; the gather of step k+2 goes into step k's buffer: it waits for whoever unpacked
    that result (Gathered.consumed), and the old result is marked stale -- unpack() of a stale result raises instead of
    returning a later step's bytes.  `new_event(stream)` returns an event recorded on `stream`."""

    def __init__(self, new_event):
        self.bufs = [None, None]
        self.prev = [None, None]
        self.turn = 0
        self.new_event = new_event

    def issue(self, side, tracked, gather):
        """Order `gather(out_buffer)` on `side` behind `tracked` (the tracking launch that filled the local slice) and
        behind the reader of the buffer it is about to overwrite.  Returns (result, event: the collective is done)."""
        k = self.turn
        self.turn = 1 - k
        side.wait_event(tracked)
        prev = self.prev[k]
        if prev is not None:
            if prev.consumed is not None:
                side.wait_event(prev.consumed)
            prev.stale = True
        res = gather(self.bufs[k])
        done = self.new_event(side)
        if isinstance(res, distributed.Gathered):
            self.bufs[k] = res.raw
            res.done = done              # unpack() / to_numpy() on any stream wait for the collective
            self.prev[k] = res
        return res, done


class ResidentTracker:
    """One frame pair resident in HBM; step() = what a tracker does per new frame:
    build the pyramid of the new (current) frame, then run PatchMatch over this rank's
    feature shard.  The reference frame's pyramid is the one the previous step built
    (cur of pair t is ref of pair t+1), so it is not rebuilt."""

    def __init__(self, params: capi.Params, device: int = 0, rank: int = 0, world: int = 1, concurrency: int = 1):
        if not torch.cuda.is_available():
            raise RuntimeError("ResidentTracker needs a HIP device (torch.cuda.is_available() is False)")
        self.params = params
        self.rank, self.world = rank, world
        self.dev = torch.device("cuda", device)
        torch.cuda.set_device(self.dev)
        self.ctx = capi.Context(device)
        if concurrency > 1:   # this many trackers share the device (one per camera stream): pagk_set_concurrency
            self.ctx.set_concurrency(concurrency)
        # Two explicit streams.  `main` carries the tracking launches (and, because step() makes it torch's
        # current stream, the RCCL all-gather orders after them); `side` builds the NEXT frame's pyramid while
        # the current pair is being tracked (a new frame's pyramid depends on no tracking result).  Never the
        # legacy default stream: its handle is 0, which pagk_set_stream reads as "the context's own stream",
        # and it cannot be captured into a hipGraph.
        self.main = torch.cuda.Stream(device=self.dev)
        self.side = torch.cuda.Stream(device=self.dev)
        self.ctx.set_stream(self.main.cuda_stream)
        self.cur_slot = 1           # slots 1 / 2 alternate as "current frame"
        self._pyr_ready = None      # event: pyramid of the frame to track next is built
        self._trk_done = {1: None, 2: None}  # event per slot: last tracking kernel that read it
        self._graphs = {}           # mode -> graph ids of the captured step ("graph": one; "fork", "fused": two)
        self._graph_failed = False  # capture was refused once: direct launches from then on
        self.mode_used = "serial"   # how the last step's launches were issued
        self._gather_done = None    # event: the previous step's all-gather (side stream) has read self.out
        self._last_gather = None
        self.n = 0

    def close(self):
        self.ctx.close()

    def load_pair(self, img_ref: np.ndarray, img_cur: np.ndarray):
        self.img_ref = torch.from_numpy(np.ascontiguousarray(img_ref)).to(self.dev)
        self.img_cur = torch.from_numpy(np.ascontiguousarray(img_cur)).to(self.dev)
        h, w = img_ref.shape
        self.w, self.h = w, h
        L = self.params.pyramids
        self.ctx.frame_set_device(0, self.img_ref.data_ptr(), w, h, w, L)
        self.ctx.frame_set_device(1, self.img_cur.data_ptr(), w, h, w, L)
        self.ctx.frame_set_device(2, self.img_cur.data_ptr(), w, h, w, L)
        self.cur_slot, self._pyr_ready = 1, None
        self._drop_graph()
        self._settle()

    def set_current_image(self, img_cur: np.ndarray):
        """The next frame of the stream: new bytes into the SAME device buffer (captured graphs stay valid), ordered
        on `main` after the launches that still read the old frame."""
        with torch.cuda.stream(self.main):
            self.img_cur.copy_(torch.from_numpy(np.ascontiguousarray(img_cur)).to(self.dev, non_blocking=False))

    def _settle(self):
        """Set-up work ran on torch's current stream and on `main`: let both finish before steps start."""
        torch.cuda.synchronize(self.dev)

    def _drop_graph(self):
        for ids in self._graphs.values():
            for gid in ids:
                self.ctx.graph_destroy(gid)
        self._graphs = {}
        if getattr(self, "_live", None) is not None:
            self.ctx.graph_destroy(self._live[1])
            self._live = None

    @property
    def _graph(self):
        """Graph ids of the default mode (None before its first step)."""
        return self._graphs.get("graph")

    def set_features(self, pt_ref, pt_init, affine, status_in):
        """Takes the FULL feature arrays; keeps this rank's contiguous shard on the device."""
        self.n = int(pt_ref.shape[0])
        lo, hi = distributed.shard_range(self.n, self.rank, self.world)
        self.lo, self.hi = lo, hi
        m = distributed.shard_size(self.n, self.world)

        def up(a, width):
            t = torch.zeros((max(m, 1), width) if width > 1 else (max(m, 1),), dtype=torch.from_numpy(a).dtype,
                            device=self.dev)
            if hi > lo:
                t[:hi - lo] = torch.from_numpy(np.ascontiguousarray(a[lo:hi])).to(self.dev)
            return t

        same_shape = getattr(self, "d_pt_ref", None) is not None and self.d_pt_ref.shape[0] == max(m, 1) \
            and getattr(self, "_n_alloc", None) == self.n
        if same_shape:
            # a stream of frames with a fixed feature capacity (unused entries carry status_in = 0): new
            # values go into the SAME device arrays, so a captured graph stays valid
            with torch.cuda.stream(self.main):
                for dst, a, width in ((self.d_pt_ref, pt_ref, 2), (self.d_pt_init, pt_init, 2),
                                      (self.d_affine, affine, 4), (self.d_status, status_in, 1)):
                    if hi > lo:
                        dst[:hi - lo].copy_(torch.from_numpy(np.ascontiguousarray(a[lo:hi])).to(self.dev))
                self.ctx.prio_hint_reset()   # new features in the slots: last launch's iteration counts forecast nothing
            self._settle()
            return
        self.d_pt_ref = up(pt_ref, 2)
        self.d_pt_init = up(pt_init, 2)
        self.d_affine = up(affine, 4)
        self.d_status = up(status_in, 1)
        self.out = distributed.alloc_device_outputs(m, self.dev)
        self._n_alloc = self.n
        self._drop_graph()
        with torch.cuda.stream(self.main):
            self.ctx.prio_hint_reset()
        self._settle()

    def rebuild_current_pyramid(self, slot: int = 1):
        self.ctx.frame_set_device(slot, self.img_cur.data_ptr(), self.w, self.h, self.w, self.params.pyramids)

    def track_shard(self, slot: int = 1):
        self.ctx.track_device(self.params, 0, slot, self.hi - self.lo, self.d_pt_ref, self.d_pt_init, self.d_affine,
                              self.d_status, self.out)

    def _prefetch_pyramid(self, slot: int):
        """Build the pyramid of the next 'current' frame into `slot` on the side stream."""
        with torch.cuda.stream(self.side):
            if self._trk_done[slot] is not None:
                self.side.wait_event(self._trk_done[slot])   # the kernel that last read this slot
            self.ctx.set_stream(self.side.cuda_stream)
            self.rebuild_current_pyramid(slot)
            ev = torch.cuda.Event()
            ev.record(self.side)
        self.ctx.set_stream(self.main.cuda_stream)
        return ev

    def step(self, gather: bool = True, mode: str = "graph"):
        """One pass of the hot path over this rank's shard (+ the result all-gather): pyramid of the
        current frame, then PatchMatch.  `mode` only chooses how the two launches reach the GPU; every
        mode builds exactly one pyramid and runs one tracking launch per step (measured on MI355X,
        752x480 / 1000 features, tools/step_modes.py, profiles/r01_step_modes.log):
          "graph"   (default) one hipGraphLaunch replaying [pyramid -> PatchMatch], captured on first use
                    (BASELINE configs[4]: "hipGraph-captured iterate"): no inter-launch gap, 121.7 us;
          "serial"  the same two launches issued directly on one stream: 132.9 us (5 us gap per launch);
          "streams" pyramid of step k+1's frame on a side stream while step k tracks, ordered by events:
                    134.6 us -- a cross-stream event wait costs more than the 7.7 us pyramid it hides;
          "fork"    that overlap as two branches of one graph: 143.6 us;
          "fused"   the next frame's pyramid as trailing workgroups of the tracking launch itself
                    (pagk_track_device_fused), one single-node graph per parity: the pyramid costs no launch and no
                    gap.  Like "streams" it needs frame k+1 while pair (k-1, k) is tracked.
        What comes back without a collective is plain VIEWS of the tracker's output buffers, written by launches on `main`:
        read them after synchronize() or on `main` (a Gathered, from the sharded step, orders its reader by itself)."""
        gather = gather and not mode.endswith("-nogather")
        mode = mode.replace("-nogather", "")
        graph = {"graph": True, "fork": "fork", "fused": "fused"}.get(mode, False)
        overlap = mode == "streams"
        if mode not in ("graph", "fork", "fused", "serial", "streams"):
            raise ValueError(mode)
        collective = gather and (self.world > 1 or distributed.FORCE_COLLECTIVE)
        if collective:
            return self._sharded_step(mode)
        with torch.cuda.stream(self.main):
            if graph and not self._graph_failed:
                try:
                    self._graph_step(fork=(graph == "fork"), fused=(graph == "fused"))
                except capi.PagkError as e:
                    # capture refused by the runtime (never seen on MI355X / ROCm 7.2): keep going with the same two
                    # launches issued directly -- still the HIP path -- and say so
                    import sys
                    print(f"pagk: hipGraph capture failed ({e}); step() falls back to direct launches", file=sys.stderr)
                    self._graph_failed = True
                    self._drop_graph()
                    self.ctx.set_stream(self.main.cuda_stream)
                    self.mode_used = "serial"
                    self.rebuild_current_pyramid(1)
                    self.track_shard(1)
                else:
                    self.mode_used = mode
            elif graph:
                self.mode_used = "serial"
                self.rebuild_current_pyramid(1)
                self.track_shard(1)
            elif not overlap:
                self.mode_used = "serial"
                self.rebuild_current_pyramid(1)
                self.track_shard(1)
            else:
                self.mode_used = "streams"
                if self._pyr_ready is None:                       # first step: nothing prefetched yet
                    self._pyr_ready = self._prefetch_pyramid(self.cur_slot)
                self.main.wait_event(self._pyr_ready)
                slot = self.cur_slot
                self.track_shard(slot)
                done = torch.cuda.Event()
                done.record(self.main)
                self._trk_done[slot] = done
                self.cur_slot = 3 - slot                          # 1 <-> 2
                self._pyr_ready = self._prefetch_pyramid(self.cur_slot)
        return {name: self.out[name][:self.hi - self.lo] for name, _, _ in distributed.FIELDS}

    def _sharded_step(self, mode: str):
        """A step of the sharded path (world > 1): pyramid, this rank's block of features, then the one exchange of
        the path -- the all-gather of the packed result slices -- on the SIDE stream, so that it runs beside the next
        step's pyramid; the next step's tracking launch waits for it (it rewrites the slice the gather reads, and in
        a tracker its inputs derive from the gathered results, src/gyro_aided_tracker.cpp:289-341).  The tracking
        launch is replayed from a one-node hipGraph when `mode` is a graph mode."""
        with torch.cuda.stream(self.main):
            self.rebuild_current_pyramid(1)                        # needs no result of the previous step
            if self._gather_done is not None:
                self.main.wait_event(self._gather_done)
            if mode in ("graph", "fused", "fork") and not self._graph_failed:
                if "track" not in self._graphs:
                    self.track_shard(1)                            # warm-up
                    self.main.synchronize()
                    try:
                        self.ctx.graph_begin()
                        try:
                            self.track_shard(1)
                        finally:
                            self._graphs["track"] = (self.ctx.graph_end(),)
                    except capi.PagkError:
                        self._graph_failed = True
                        self._graphs.pop("track", None)
                if "track" in self._graphs:
                    self.ctx.graph_launch(self._graphs["track"][0])
                    self.mode_used = "graph"
                else:
                    self.track_shard(1)
                    self.mode_used = "serial"
            else:
                self.track_shard(1)
                self.mode_used = "serial"
            tracked = torch.cuda.Event()
            tracked.record(self.main)
        ring = getattr(self, "_gather_ring", None)
        if ring is None:
            ring = self._gather_ring = GatherRing(_event_on)
        with torch.cuda.stream(self.side):
            res, self._gather_done = ring.issue(self.side, tracked, lambda out: distributed.all_gather_results(self.out, self.n, out=out))
        self._last_gather = res
        return res

    def step_live(self, host_frame: "torch.Tensor"):
        """The step of a live camera loop INCLUDING the frame's way onto the device: `host_frame` is the camera's PINNED
        uint8 buffer (h x w); the graph [host -> device copy of that buffer -> pyramid -> PatchMatch] is captured on
        first use (pagk_frame_upload_pinned is capturable) and replayed with one launch per frame -- the caller writes
        the new frame into the same pinned buffer before each call.  (Examples/Demo/RealSenseD435i.cpp:199-321 is the
        loop this stands for: grab, convert, track.)  Returns the rank's device outputs; nothing is synchronised."""
        key = (host_frame.data_ptr(), tuple(host_frame.shape))
        if getattr(self, "_live", None) is None or self._live[0] != key:
            if getattr(self, "_live", None) is not None:
                self.ctx.graph_destroy(self._live[1])
            if not host_frame.is_pinned():
                raise ValueError("step_live needs the frame in pinned host memory")
            h, w = host_frame.shape
            with torch.cuda.stream(self.main):
                self.ctx.frame_upload_pinned(1, host_frame.data_ptr(), w, h, host_frame.stride(0), self.params.pyramids)
                self.track_shard(1)                      # warm-up: allocations, kernel attributes
                self.main.synchronize()
                self.ctx.graph_begin()
                try:
                    self.ctx.frame_upload_pinned(1, host_frame.data_ptr(), w, h, host_frame.stride(0), self.params.pyramids)
                    self.track_shard(1)
                finally:
                    gid = self.ctx.graph_end()
            self._live = (key, gid, host_frame)          # (keeps the pinned buffer alive as long as the graph)
        self.ctx.graph_launch(self._live[1])
        self.mode_used = "live"
        return self.out

    def finish(self):
        """Order everything issued so far (tracking on `main`, the last gather on `side`) before the caller's
        stream-wide synchronisation."""
        if self._gather_done is not None:
            self.main.wait_event(self._gather_done)

    def gather_report(self, reps: int = 20) -> dict:
        """The all-gather by itself: average duration from events on the stream it runs on."""
        ts = []
        with torch.cuda.stream(self.side):
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(self.side)
                distributed.all_gather_results(self.out, self.n, out=(self._gather_ring.bufs[0] if getattr(self, "_gather_ring", None) else None))
                e1.record(self.side)
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
        return {"gather_ms": float(np.mean(ts[2:])) if len(ts) > 2 else float(np.mean(ts)),
                "bytes_per_rank": int(self.out["_buf"].numel()), "ranks": self.world}

    def track_shard_fused(self, cur: int):
        """PatchMatch(0, cur) and, in the same launch, the pyramid of the next frame into the other slot."""
        self.ctx.track_device_fused(self.params, 0, cur, self.hi - self.lo, self.d_pt_ref, self.d_pt_init, self.d_affine,
                                    self.d_status, self.out, 3 - cur, self.img_cur.data_ptr(), self.w, self.h, self.w,
                                    self.params.pyramids)

    def _graph_step(self, fork: bool, fused: bool = False):
        """Replay (capturing on first use) the step as a hipGraph.  Linear form: [pyramid(slot 1) ->
        PatchMatch(0, 1)].  Fork form: two graphs, one per parity, each [PatchMatch(0, cur) || pyramid(next)]
        -- the side-stream prefetch of step() expressed as two independent branches of one graph.  Fused form:
        two single-node graphs, [PatchMatch(0, cur) + pyramid(next frame -> the other slot) in one launch]."""
        key = "fused" if fused else ("fork" if fork else "graph")
        if key not in self._graphs:
            self.rebuild_current_pyramid(1)      # warm-up: allocations, kernel attributes
            self.rebuild_current_pyramid(2)
            self.track_shard(1)
            self.main.synchronize()
            ids = []
            if fused:
                self.track_shard_fused(1)        # warm-up of the fused kernel
                self.main.synchronize()
                for cur in (1, 2):
                    self.ctx.graph_begin()
                    try:
                        self.track_shard_fused(cur)
                    finally:
                        ids.append(self.ctx.graph_end())
            elif not fork:
                self.ctx.graph_begin()
                try:
                    self.rebuild_current_pyramid(1)
                    self.track_shard(1)
                finally:
                    ids.append(self.ctx.graph_end())
            else:
                for cur in (1, 2):
                    self.ctx.graph_begin()       # capture starts on `main`
                    try:
                        e1 = torch.cuda.Event()
                        e1.record(self.main)
                        self.side.wait_event(e1)                 # fork: `side` joins the capture
                        self.ctx.set_stream(self.side.cuda_stream)
                        self.rebuild_current_pyramid(3 - cur)    # next frame's pyramid
                        self.ctx.set_stream(self.main.cuda_stream)
                        self.track_shard(cur)
                        e2 = torch.cuda.Event()
                        e2.record(self.side)
                        self.main.wait_event(e2)                 # join
                    finally:
                        self.ctx.set_stream(self.main.cuda_stream)
                        ids.append(self.ctx.graph_end())
            self._graphs[key] = tuple(ids)
            self.cur_slot = 1
        ids = self._graphs[key]
        if len(ids) == 1:
            self.ctx.graph_launch(ids[0])
        else:
            # both slots hold a valid pyramid whenever the mode changes: every parity graph leaves them so
            self.ctx.graph_launch(ids[self.cur_slot - 1])
            self.cur_slot = 3 - self.cur_slot

    def synchronize(self):
        """Wait for everything step() has issued (tracking on `main`, prefetch / gather on `side`); then ask the library
        whether one of those launches failed -- these are torch's stream synchronisations, not pagk_sync, so the error
        word of the level-by-level launches (include/pagk.h: pagk_check_launch) would otherwise never be read."""
        self.main.synchronize()
        self.side.synchronize()
        self.ctx.check_launch()


class CameraBatch:
    """k camera streams that share ONE GPU, stepped as one launch: BASELINE configs[4], "batched multi-camera: concurrent
    streams, hipGraph-captured iterate".  The reference builds one PatchMatch per tracker
    (src/gyro_aided_tracker.cpp:276-283); here every stream is a ResidentTracker (its own context: frame slots, feature
    arrays, outputs), all switched to ONE stream, and a step is [the k current frames' pyramids as one launch
    (pagk_frame_set_device_batch), then pagk_track_device_batch] -- replayed as one hipGraph after the first step, or issued directly."""

    def __init__(self, params: capi.Params, k: int, device: int = 0):
        self.params = params
        self.cams = [ResidentTracker(params, device=device) for _ in range(k)]
        self.stream = self.cams[0].main
        for c in self.cams[1:]:
            c.ctx.set_stream(self.stream.cuda_stream)   # one stream for the whole batch: nothing to order across streams
        self._graph = None
        self.mode_used = "serial"

    def close(self):
        self._drop_graph()
        for c in self.cams:
            c.close()

    def _drop_graph(self):
        if self._graph is not None:
            self.cams[0].ctx.graph_destroy(self._graph)
            self._graph = None

    def load(self, j: int, img_ref, img_cur, pt_ref, pt_init, affine, status_in):
        """Stream j's frame pair and features (any image size, any feature count)."""
        c = self.cams[j]
        c.load_pair(img_ref, img_cur)
        c.set_features(pt_ref, pt_init, affine, status_in)
        c.ctx.set_stream(self.stream.cuda_stream)
        self._drop_graph()

    def _issue(self):
        cs = self.cams
        # the k current frames' pyramids as one launch, then the k trackers' PatchMatch as one launch
        capi.Context.frame_set_device_batch([c.ctx for c in cs], [1] * len(cs), [c.img_cur.data_ptr() for c in cs],
                                            [c.w for c in cs], [c.h for c in cs], [c.w for c in cs], self.params.pyramids)
        capi.Context.track_device_batch([c.ctx for c in cs], self.params, [0] * len(cs), [1] * len(cs),
                                        [c.hi - c.lo for c in cs], [c.d_pt_ref for c in cs], [c.d_pt_init for c in cs],
                                        [c.d_affine for c in cs], [c.d_status for c in cs], [c.out for c in cs])

    def step(self, mode: str = "graph"):
        """One frame of every stream; returns the streams' output dicts (device tensors, valid once `stream` has run)."""
        lead = self.cams[0].ctx
        with torch.cuda.stream(self.stream):
            if mode == "graph":
                if self._graph is None:
                    self._issue()                      # warm-up: allocations happen outside the capture
                    self.stream.synchronize()
                    lead.graph_begin()
                    try:
                        self._issue()
                    finally:
                        self._graph = lead.graph_end()
                lead.graph_launch(self._graph)
            else:
                self._issue()
        self.mode_used = mode
        return [c.out for c in self.cams]

    def synchronize(self):
        self.stream.synchronize()
        for c in self.cams:
            c.ctx.check_launch()


def _carve(buf: torch.Tensor, fields):
    """Typed views into one byte buffer: fields = [(name, dtype, rows, cols)], every block 256-byte aligned."""
    out, off = {}, 0
    for name, dt, rows, cols in fields:
        nbytes = torch.empty(0, dtype=dt).element_size() * rows * cols
        v = buf[off:off + nbytes].view(dt)
        out[name] = v.view(rows, cols) if cols > 1 else v
        off += (nbytes + 255) // 256 * 256
    return out


def _carve_size(fields) -> int:
    return sum((torch.empty(0, dtype=dt).element_size() * rows * cols + 255) // 256 * 256 for _, dt, rows, cols in fields)


class FrameResult:
    """What one SequenceTracker step leaves behind: the keypoints of the next pair (keys, keys_un, keys_normal,
    index_in_last, live: `cap` entries each) and the hand-over's state words, as device tensors, with the event that was
    recorded behind the work that produces them.  to_numpy() waits for that event (and for nothing issued later).  A
    tracker with a detector adds the detector's info words ("info")."""

    FIELDS = ("keys", "keys_un", "keys_normal", "index_in_last", "live", "state")

    def __init__(self, tensors: dict, event, side, snapshot: bool):
        self.tensors, self.event, self._side, self.snapshot = tensors, event, side, snapshot

    def to_numpy(self) -> dict:
        with torch.cuda.stream(self._side):
            self._side.wait_event(self.event)
            host = {k: self.tensors[k].to("cpu", non_blocking=False) for k in self.FIELDS}
            if "info" in self.tensors:
                host["info"] = self.tensors["info"].to("cpu", non_blocking=False)
        out = {k: v.numpy() for k, v in host.items()}
        out.update(zip(capi.HANDOVER_STATE_FIELDS, (int(v) for v in out["state"][:5])))
        return out


class SequenceTracker:
    """A tracker's per-frame loop with everything between two frame pairs on the device (reference
    Examples/Demo/RealSenseD435i.cpp:199-321): step() enqueues
        [frame -> pyramid -> pagk_gyro_predict_device_live -> pagk_track_device -> pagk_post_filter_device ->
         pagk_geometry_validation_device -> pagk_frame_handover_device]
    on one stream, with no host synchronisation and no device-to-host copy.  Every launch is sized by the fixed
    capacity `cap`; the live count stays in device memory (dead slots are status_in = 0 for the tracking kernels).
    What changes from frame to frame -- the image, the nine rotation floats, the candidate list and its length -- goes
    through ONE pinned block and one host-to-device copy into a fixed device block in front of the frame's work.
    The even and the odd frame (they differ in their frame slots and key-array sets) are captured as two graphs after
    one direct run of each; mode="direct" issues the same calls without a graph.

    target_n = Frame::mN, new_point_ratio = th of mThresholdOfPredictNewKeyPoint = mN * th (src/frame.cpp:79).
    fit_params None leaves the geometry validation out.

    detector (a capi.DetectParams) closes the loop: the hand-over becomes pagk_frame_handover_detect_device, which
    detects the top-up on the current frame under the mask it has just built (Frame::DetectKeyPoints, src/frame.cpp:
    156-218), so start() and step() take no candidate list and a sequence starts with no keypoints from outside.
    detector=None is the loop with the application's own candidates.  A capi.FastParams as the detector selects the
    branch the reference's front-ends take instead (ORBextractor::DetectFeatures, src/ORBextractor.cc:1148-1205: FAST in
    cells, then the quadtree): the hand-over becomes pagk_frame_handover_fast_device.

    rectify = (map_x, map_y, rectify_params, (src_height, src_width)) puts the reference's per-frame cv::remap and the
    RGB-to-gray step of Frame::Frame (Examples/Demo/RealSenseD435i.cpp:202, src/frame.cpp:81-87) in front of the pyramid,
    on the device: start() and step() then take the RAW camera frame (src_height x src_width, or x channels), the maps
    (float32, height x width) are converted once here, and each frame slot holds its own rectified image
    (pagk_frame_rectify_device instead of pagk_frame_set_device).  rectify=None issues exactly the calls described above."""

    RING = 4   # pinned input blocks: one is rewritten only after the copy that read it, four frames earlier, has run

    def __init__(self, params: capi.Params, width: int, height: int, cap: int, target_n: int, new_point_ratio: float,
                 fit_params: "capi.FitParams | None" = None, *, device: int = 0, cand_cap: int = 1024, sigma: float = 1.0,
                 detector: "capi.DetectParams | capi.FastParams | None" = None, rectify=None):
        if not torch.cuda.is_available():
            raise RuntimeError("SequenceTracker needs a HIP device (torch.cuda.is_available() is False)")
        if cap < target_n or target_n < 1 or (detector is None and cand_cap < 1):
            raise ValueError("cap >= target_n >= 1 and cand_cap >= 1 are required")
        self.params, self.fit_params, self.sigma, self.detector = params, fit_params, float(sigma), detector
        self.w, self.h, self.cap, self.target_n, self.cand_cap = int(width), int(height), int(cap), int(target_n), int(cand_cap)
        self.threshold = float(target_n * new_point_ratio)
        self.dev = torch.device("cuda", device)
        torch.cuda.set_device(self.dev)
        self.ctx = capi.Context(device)
        self.main = torch.cuda.Stream(device=self.dev)   # never the legacy default stream (it cannot be captured)
        self.side = torch.cuda.Stream(device=self.dev)   # readers of a FrameResult
        self.ctx.set_stream(self.main.cuda_stream)
        u8, f32, f64, i32 = torch.uint8, torch.float32, torch.float64, torch.int32
        n = self.cap
        self.rectify = None
        img_rows, img_cols = self.h, self.w
        if rectify is not None:
            map_x, map_y, rp, (hs, ws) = rectify
            if np.shape(map_x) != (self.h, self.w) or np.shape(map_y) != (self.h, self.w):
                raise ValueError("the maps must have the tracker's size (height x width)")
            self.ctx.rectify_set_maps(np.ascontiguousarray(map_x, np.float32), np.ascontiguousarray(map_y, np.float32))
            self.rectify = (rp, int(ws), int(hs), int(rp.channels))
            img_rows, img_cols = int(hs), int(ws) * int(rp.channels)   # the input block's "img" is the raw frame
        self._in_fields = [("img", u8, img_rows, img_cols), ("rot", f32, 9, 1)]
        if detector is None:   # with a detector no candidate list exists: the input block is the image and the rotation
            self._in_fields += [("n_cand", i32, 1, 1), ("cand", f32, self.cand_cap, 2)]
        nbytes = _carve_size(self._in_fields)
        self._d_in_buf = torch.zeros(nbytes, dtype=u8, device=self.dev)
        self.d_in = _carve(self._d_in_buf, self._in_fields)
        self._pinned = [torch.zeros(nbytes, dtype=u8).pin_memory() for _ in range(self.RING)]
        self._pinned_views = [_carve(b, self._in_fields) for b in self._pinned]
        self._pinned_free = [None] * self.RING
        set_fields = [("keys", f32, n, 2), ("keys_un", f32, n, 2), ("keys_normal", f32, n, 2), ("index_in_last", i32, n, 1),
                      ("live", u8, n, 1)]
        self._set_bufs = [torch.zeros(_carve_size(set_fields), dtype=u8, device=self.dev) for _ in range(2)]
        self._set_fields = set_fields
        self.sets = [_carve(b, set_fields) for b in self._set_bufs]
        work = [("pu", f32, n, 2), ("pd", f32, n, 2), ("st_in", u8, n, 1), ("aff", f32, n, 4), ("pt_un", f32, n, 2),
                ("pt_dist", f32, n, 2), ("status", u8, n, 1), ("pix_err", f64, n, 1), ("dist_pred", f64, n, 1),
                ("st", u8, n, 1), ("pp", f32, n, 2), ("ppu", f32, n, 2), ("kept", i32, 1, 1), ("th", f64, 2, 1),
                ("cnt", i32, 1, 1), ("score", f32, 1, 1), ("zero", u8, n, 1)]
        self._work_buf = torch.zeros(_carve_size(work), dtype=u8, device=self.dev)
        self.wk = _carve(self._work_buf, work)
        self.wk["aff"].copy_(torch.tensor([1.0, 0.0, 0.0, 1.0], device=self.dev).repeat(n, 1))
        self.out = {k: self.wk[k] for k in ("pt_un", "pt_dist", "status", "pix_err", "dist_pred")}
        self.state = torch.zeros(capi.HANDOVER_STATE_WORDS, dtype=i32, device=self.dev)
        self.info = torch.zeros(capi.DETECT_INFO_WORDS, dtype=i32, device=self.dev) if detector is not None else None
        torch.cuda.synchronize(self.dev)
        self.frame = -1          # index of the last frame handed in
        self._turn = 0
        self._graphs = {}        # parity -> graph id
        self._direct_done = set()
        self.mode_used = None

    def close(self):
        for gid in self._graphs.values():
            self.ctx.graph_destroy(gid)
        self._graphs = {}
        self.ctx.close()

    # -- inputs ------------------------------------------------------------------------------------------------
    def _feed(self, img, rot9, candidates):
        """This frame's inputs into the next pinned block, then one asynchronous copy into the fixed device block."""
        k = self._turn
        self._turn = (k + 1) % self.RING
        if self._pinned_free[k] is not None:
            self._pinned_free[k].synchronize()   # the copy issued RING frames ago has read this block (flow control only)
        pv = self._pinned_views[k]
        img = np.asarray(img)
        if self.rectify is not None:
            _, ws, hs, cn = self.rectify
            if img.dtype != np.uint8 or img.shape not in (((hs, ws, cn),) if cn > 1 else ((hs, ws), (hs, ws, 1))):
                raise ValueError("frame must be the raw uint8 frame, src_height x src_width (x channels)")
            img = img.reshape(hs, ws * cn)
        elif img.shape != (self.h, self.w) or img.dtype != np.uint8:
            raise ValueError("frame must be a uint8 array of the tracker's size")
        pv["img"].numpy()[...] = img
        if rot9 is not None:
            pv["rot"].numpy()[...] = np.asarray(rot9, np.float32).reshape(9)
        if self.detector is None:
            cand = np.asarray(candidates, np.float32).reshape(-1, 2)
            if cand.shape[0] > self.cand_cap:
                raise ValueError("more candidates than cand_cap")
            pv["cand"].numpy()[:cand.shape[0]] = cand
            pv["n_cand"].numpy()[0] = cand.shape[0]
        self._d_in_buf.copy_(self._pinned[k], non_blocking=True)
        self._pinned_free[k] = _event_on(self.main)

    # -- the frame's launches ----------------------------------------------------------------------------------
    def _frame(self, slot: int):
        """The frame in the fixed device block into frame slot `slot`: its pyramid, behind the rectification if there is one."""
        if self.rectify is not None:
            rp, ws, hs, cn = self.rectify
            self.ctx.frame_rectify_device(slot, rp, self.d_in["img"].data_ptr(), ws, hs, ws * cn, self.params.pyramids)
            return
        self.ctx.frame_set_device(slot, self.d_in["img"].data_ptr(), self.w, self.h, self.w, self.params.pyramids)

    def _handover(self, status, pp, ppu, dst, slot: int):
        if isinstance(self.detector, capi.FastParams):   # FAST in cells and the quadtree on the frame in `slot`
            self.ctx.frame_handover_fast_device(self.params, self.w, self.h, self.cap, self.target_n, self.threshold,
                                                status, pp, ppu, self.detector, slot, dst["keys"], dst["keys_un"],
                                                dst["keys_normal"], dst["index_in_last"], dst["live"], None,
                                                self.state, self.info)
            return
        if self.detector is not None:   # the candidates are detected on the frame in `slot`, under this call's mask
            self.ctx.frame_handover_detect_device(self.params, self.w, self.h, self.cap, self.target_n, self.threshold,
                                                  status, pp, ppu, self.detector, slot, dst["keys"], dst["keys_un"],
                                                  dst["keys_normal"], dst["index_in_last"], dst["live"], None,
                                                  self.state, self.info)
            return
        self.ctx.frame_handover_device(self.params, self.w, self.h, self.cap, self.target_n, self.threshold, status, pp, ppu,
                                       self.cand_cap, self.d_in["n_cand"], self.d_in["cand"], dst["keys"], dst["keys_un"],
                                       dst["keys_normal"], dst["index_in_last"], dst["live"], None, self.state)

    def _issue(self, p: int):
        """The work of a frame of parity p: frame slot p is the current frame, slot 1 - p the reference; key set 1 - p
        holds the reference keypoints, set p receives the next pair's."""
        c, pr, wk = self.ctx, self.params, self.wk
        ref, dst = self.sets[1 - p], self.sets[p]
        self._frame(p)
        if pr.has_gyro_predict_initial:
            c.gyro_predict_device_live(pr, self.w, self.h, self.d_in["rot"], self.cap, ref["keys_un"], ref["live"],
                                       wk["pu"], wk["pd"], wk["st_in"], wk["aff"])
            c.track_device(pr, 1 - p, p, self.cap, ref["keys_un"], wk["pu"], wk["aff"], wk["st_in"], self.out)
        else:   # no prediction: the live mask is the tracking kernels' status_in
            c.track_device(pr, 1 - p, p, self.cap, ref["keys_un"], ref["keys_un"], wk["aff"], ref["live"], self.out)
        c.post_filter_device(self.cap, pr.half_patch, wk["status"], wk["pix_err"], wk["dist_pred"], wk["pt_dist"],
                             wk["pt_un"], wk["st"], wk["pp"], wk["ppu"], wk["kept"], wk["th"])
        if self.fit_params is not None:
            c.geometry_validation_device(self.fit_params, self.cap, ref["keys_un"], wk["ppu"], wk["st"], self.sigma,
                                         wk["cnt"], wk["score"])
        self._handover(wk["st"], wk["pp"], wk["ppu"], dst, p)

    def _result(self, p: int, snapshot: bool) -> FrameResult:
        if snapshot:   # two device-to-device copies: the set's block and the state words
            t = _carve(self._set_bufs[p].clone(), self._set_fields)
            t["state"] = self.state.clone()
            if self.info is not None:
                t["info"] = self.info.clone()
        else:          # views: valid until the frame after next rewrites this set
            t = dict(self.sets[p])
            t["state"] = self.state
            if self.info is not None:
                t["info"] = self.info
        return FrameResult(t, _event_on(self.main), self.side, snapshot)

    def _check_list(self, candidates):
        """A candidate list is required without a detector (an empty array for "none") and refused with one."""
        if self.detector is not None and candidates is not None:
            raise ValueError("this tracker detects its own keypoints (detector=...): pass no candidate list")
        if self.detector is None and candidates is None:
            raise TypeError("a tracker without a detector needs the frame's candidate list (an empty array for none)")

    def start(self, img, candidates=None, snapshot: bool = True) -> FrameResult:
        """The first frame (Examples/Demo/RealSenseD435i.cpp:221-235): its pyramid into slot 0, and the first-frame
        hand-over -- an all-zero status -- takes the first target_n in-image candidates into key set 0 (with a
        detector: the target_n strongest corners of the frame that keep their distance)."""
        self._check_list(candidates)
        with torch.cuda.stream(self.main):
            self.state.zero_()
            self._feed(img, None, candidates)
            self._frame(0)
            self._handover(self.wk["zero"], self.wk["pp"], self.wk["ppu"], self.sets[0], 0)
            self.frame = 0
            self.mode_used = "direct"
            return self._result(0, snapshot)

    def step(self, img, rot9, candidates=None, mode: str = "graph", snapshot: bool = True) -> FrameResult:
        """Frame k >= 1: tracks pair (k-1, k) and hands over to pair (k, k+1).  rot9 = rows 0 and 1 of K R K^-1 followed
        by the third row of R (pagk_gyro_predict_device_rot).  Nothing is synchronised; the result carries its event."""
        if self.frame < 0:
            raise RuntimeError("start() hands in the first frame")
        if mode not in ("graph", "direct"):
            raise ValueError(mode)
        self._check_list(candidates)
        k = self.frame + 1
        p = k & 1
        with torch.cuda.stream(self.main):
            self._feed(img, rot9, candidates)
            if mode == "graph" and p in self._direct_done:
                if p not in self._graphs:
                    self.ctx.graph_begin()
                    try:
                        self._issue(p)
                    finally:
                        self._graphs[p] = self.ctx.graph_end()
                self.ctx.graph_launch(self._graphs[p])
                self.mode_used = "graph"
            else:   # also the first frame of each parity in graph mode: allocations happen outside a capture
                self._issue(p)
                self._direct_done.add(p)
                self.mode_used = "direct"
            self.frame = k
            return self._result(p, snapshot)

    def synchronize(self):
        self.main.synchronize()
        self.side.synchronize()
        self.ctx.check_launch()



class DeviceSequence:
    """The frame loop behind the C ABI (pagk_sequence_*, reference Examples/Demo/RealSenseD435i.cpp:199-321) on numpy arrays:
    the context owns the key sets, the work arrays, the pinned input ring and the two per-parity graphs, so this class keeps
    nothing but the context.  `sp` is a capi.SequenceParams (capi.sequence_params_default(...)): tracker PatchMatch,
    Lucas-Kanade or gyro-started Lucas-Kanade; detector 0 (the caller's candidate lists), 1 (Harris) or 2 (FAST).
    SequenceTracker is the same loop for a Python host that keeps its results on the device.
    With `sensor` (a capi.SequenceSensor) it is the sensor form: start(raw, t=...) and step(raw, window=...) take what the
    camera and the IMU deliver (raw frames through the context's maps, set with ctx.rectify_set_maps before; a
    capi.imu_window), and read_velocity() returns mvFlowVelocityInNormalPlane.
    With `results` (2 .. 8) the sequence has a result ring of that depth (pagk_sequence_results_create): fetch(frame) returns
    the record of any of the last `results` frames -- everything read, read_pair and read_velocity deliver, track ids and
    ages -- as a dict of copies without draining the stream, poll(frame) whether its copy has arrived."""

    def __init__(self, sp: "capi.SequenceParams", device: int = 0, ctx: "capi.Context | None" = None,
                 sensor: "capi.SequenceSensor | None" = None, results: "int | None" = None):
        self._own = ctx is None
        self.ctx = capi.Context(device) if ctx is None else ctx
        self.sp = sp
        self.sensor = sensor
        try:
            if sensor is None:
                self.ctx.sequence_create(sp)
            else:
                self.ctx.sequence_create_sensor(sp, sensor)
        except Exception:
            if self._own:
                self.ctx.close()
            raise
        self._open = True
        if results is not None:
            try:
                self.ctx.sequence_results_create(int(results))
            except Exception:
                self.close()
                raise

    def start(self, frame, candidates=None, t: "float | None" = None):
        if self.sensor is not None:
            if t is None:
                raise ValueError("a sensor sequence starts with the frame's time stamp")
            return self.ctx.sequence_start_sensor(frame, t, candidates)   # (a raw frame is taken as it is: rows may be padded)
        self.ctx.sequence_start(np.ascontiguousarray(frame, np.uint8), candidates)

    def step(self, frame, rot9=None, candidates=None, mode: str = "graph", window=None):
        if mode not in ("graph", "direct"):
            raise ValueError(mode)
        m = capi.SEQ_GRAPH if mode == "graph" else capi.SEQ_DIRECT
        if self.sensor is not None:
            if window is None or rot9 is not None:
                raise ValueError("a sensor sequence steps with an IMU window, not with rot9")
            return self.ctx.sequence_step_sensor(frame, window, candidates, m)
        self.ctx.sequence_step(np.ascontiguousarray(frame, np.uint8), rot9, candidates, m)

    def read_velocity(self, cap: "int | None" = None):
        return self.ctx.sequence_read_velocity(int(self.sp.cap if cap is None else cap))

    def read(self, cap: "int | None" = None) -> dict:
        return self.ctx.sequence_read(int(self.sp.cap if cap is None else cap))

    def read_pair(self, cap: "int | None" = None) -> dict:
        return self.ctx.sequence_read_pair(int(self.sp.cap if cap is None else cap))

    def status(self) -> dict:
        return self.ctx.sequence_status()

    def fetch(self, frame: int) -> dict:
        return self.ctx.sequence_fetch(frame)

    def poll(self, frame: int) -> bool:
        return self.ctx.sequence_poll(frame)

    def close(self):
        if self._open:
            self._open = False
            self.ctx.sequence_destroy()
            if self._own:
                self.ctx.close()


class DeviceSequenceGroup:
    """k cameras stepped together (pagk_sequence_group_*): k contexts on one device, each with a plain sequence of the
    parameters `sp` (PatchMatch, the caller's candidate lists; with or without the gyro prediction and the validation), every
    stage of a frame issued once for the whole rig.  Per camera the results are, byte for byte, those of a DeviceSequence
    fed the same frames, rot9 and candidates.  frames, rot9s and cands are sequences of k numpy arrays (rot9s may be None
    when nothing predicts); read(j) and read_pair(j) return camera j's arrays.
    With `sensor` (a capi.SequenceSensor) it is the sensor form (pagk_sequence_group_*_sensor): k sensor sequences, detector 0
    or 2 (FAST); `rbc` gives every camera its own Rbc (k arrays of nine numbers; default: the block's), `maps` its own
    rectification maps (k pairs (map_x, map_y), required with raw = 1).  start(frames, cands, t=[...]) takes the raw frames and
    their time stamps, step(frames, windows=[...], cands=...) one capi.ImuWindow per camera; cands is None with detector 2;
    read_velocity(j) returns camera j's flow velocities.
    With `results` (2 .. 8) every member has a result ring of that depth: fetch(j, frame) and poll(j, frame) are camera j's.
    With sp.tracker == capi.SEQ_LK it is the Lucas-Kanade group (pagk_sequence_group_create_lk): tracker type 0, the image-only
    baseline, or with lk_initial_flow Lucas-Kanade started from the gyro prediction; plain members with the caller's lists,
    sensor members with detector 0 or 2.  Everything else -- start, step, the read calls, the rings -- is as above."""

    def __init__(self, sp: "capi.SequenceParams", k: int, device: int = 0, sensor: "capi.SequenceSensor | None" = None,
                 rbc=None, maps=None, results: "int | None" = None):
        lk = sp.tracker == capi.SEQ_LK
        if lk:
            ok = capi.sequence_group_lk_check(sp, sensor)
        else:
            ok = capi.sequence_group_check(sp) if sensor is None else capi.sequence_group_sensor_check(sp, sensor)
        if ok != capi.PAGK_OK:
            raise ValueError("pagk_sequence_group_lk_check refuses these parameters" if lk else
                             "pagk_sequence_group_check refuses these parameters" if sensor is None else
                             "pagk_sequence_group_sensor_check refuses these parameters")
        if sensor is None and (rbc is not None or maps is not None):
            raise ValueError("rbc and maps belong to the sensor form")
        if (rbc is not None and len(rbc) != k) or (maps is not None and len(maps) != k):
            raise ValueError("one Rbc and one pair of maps per camera")
        self.sp, self.k, self.sensor = sp, int(k), sensor
        self.seqs, self.group = [], None
        try:
            for j in range(self.k):
                if sensor is None:
                    self.seqs.append(DeviceSequence(sp, device, results=results))
                    continue
                ctx = capi.Context(device)
                try:
                    if maps is not None:
                        ctx.rectify_set_maps(*maps[j])
                    own = sensor
                    if rbc is not None:
                        own = capi.SequenceSensor.from_buffer_copy(sensor)
                        own.Rbc = (capi.C.c_float * 9)(*[float(x) for x in np.asarray(rbc[j], np.float32).reshape(9)])
                    seq = DeviceSequence(sp, ctx=ctx, sensor=own, results=results)
                except Exception:
                    ctx.close()
                    raise
                seq._own = True          # (the context was made here: close() closes it)
                self.seqs.append(seq)
            self.group = capi.SequenceGroup([s.ctx for s in self.seqs], sensor=sensor is not None, lk=lk)
        except Exception:
            self.close()
            raise

    def start(self, frames, cands=None, t=None):
        if self.sensor is not None:
            if t is None:
                raise ValueError("a sensor group starts with the frames' time stamps")
            return self.group.start_sensor(list(frames), t, cands)       # (raw frames are taken as they are: rows may be padded)
        self.group.start([np.ascontiguousarray(f, np.uint8) for f in frames], cands)

    def step(self, frames, rot9s=None, cands=None, mode: str = "graph", windows=None):
        if mode not in ("graph", "direct"):
            raise ValueError(mode)
        m = capi.SEQ_GRAPH if mode == "graph" else capi.SEQ_DIRECT
        if self.sensor is not None:
            if windows is None or rot9s is not None:
                raise ValueError("a sensor group steps with IMU windows, not with rot9")
            return self.group.step_sensor(list(frames), windows, cands, m)
        self.group.step([np.ascontiguousarray(f, np.uint8) for f in frames], rot9s, cands, m)

    def read_velocity(self, j: int, cap: "int | None" = None):
        return self.seqs[j].read_velocity(cap)

    def read(self, j: int, cap: "int | None" = None) -> dict:
        return self.seqs[j].read(cap)

    def read_pair(self, j: int, cap: "int | None" = None) -> dict:
        return self.seqs[j].read_pair(cap)

    def fetch(self, j: int, frame: int) -> dict:
        return self.seqs[j].fetch(frame)

    def poll(self, j: int, frame: int) -> bool:
        return self.seqs[j].poll(frame)

    def status(self) -> dict:
        return self.group.status()

    def dissolve(self):
        """pagk_sequence_group_destroy: the members (self.seqs) are ordinary sequences again and can be stepped alone."""
        if self.group is not None:
            self.group.destroy()
            self.group = None

    def close(self):
        self.dissolve()
        for s in self.seqs:
            s.close()
        self.seqs = []
