"""R(2+1)D pipeline stages (RunnerModel plugins).

Same class names and kwargs as the reference (reference: models/r2p1d/
model.py:20-296) so reference configs resolve unchanged through
``load_class``:

``R2P1DLoader``        video path -> clips (sampler + decoder)       [C16]
``R2P1DRunner``        any layer range [start_index, end_index]      [C14]
``R2P1DSingleStep``    loader + whole model in one stage             [C19]
``R2P1DAggregator``    per-video sum/argmax, segment re-join         [C20]
``LargeSmallSelector`` 15-clip videos -> queue 1, others -> queue 0   [C9]
``R2P1DVideoPathIterator`` directory walk, or synthetic paths         [C12]

MI355X-specific behaviour (documented deviations):

* Weights are random-init (seeded, identical in every replica) unless
  ``ckpt_path`` points at a reference checkpoint (loaded with
  ``torch.load(weights_only=True)``); the reference's hard-coded site paths
  are unavailable.
* Stage boundaries are NDHWC (channels padded to 4 for fp32, 8 for bf16)
  instead of NCDHW; runners also accept the reference NCDHW fp32 layout and
  convert. ``dtype`` (every stage) selects the compute precision: ``"fp32"``
  (default; the reference's precision, fp32 MFMA kernels) or ``"bf16"``.
* ``R2P1DRunner`` batches on the consumer side: with ``max_batch_videos`` > 1
  one call takes every queued video that fits ``max_clips`` rows and the
  runner pulls their slots straight into the HIP-graph input buffer
  (``gather_limits`` / ``gather_buffers``, runner.py), the in-process form of
  the reference's Batcher step (reference batcher.py:5-34).
* Runner output slots are sized from ``start_index/end_index`` (fixes the
  reference's TODO #69) and ``max_clips`` (default 15, the sampler maximum;
  the reference's 10-row slots overflow on 15-clip videos).
* Empty inputs (a 1-clip video split into 3 segments yields 0-row segments)
  return 0-row outputs instead of running the model on an empty batch.
"""
from __future__ import annotations

import json
import os
from typing import Optional, Sequence

import numpy as np
import torch

from ...ops import video as vops
from ...runner_model import RunnerModel
from ...selector import QueueSelector
from ...timecard import TimeCard, TimeCardList
from ...video_path_provider import (DirectoryLabels, DirectoryVideoPathIterator,
                                    SyntheticVideoPathIterator, VideoPathIterator)
from .decoder import make_decoder
from .engine import (GraphedEngine, R2P1DEngine, boundary_channels_p, boundary_shape,
                     check_max_clips, parse_bucket_step)
from .network import (DEFAULT_BN_EPS, DEFAULT_CLIP_LENGTH, LAYER_INPUT_CTHW,
                      R2Plus1DLayerWrapper, TVVideoResNet, check_arch, check_bn_eps,
                      check_clip_length, check_midplanes, init_random_,
                      load_reference_state_dict, load_torchvision_state_dict,
                      normalize_layer_sizes, tv_state_mids)
from .sampler import PLACEMENTS, R2P1DSampler, check_frame_step, clip_span, parse_rate, step_of

DEFAULT_MAX_CLIPS = 15
CLIP_SHAPE = (8, 112, 112)


def clip_shape(clip_length=DEFAULT_CLIP_LENGTH):
    """(frames, height, width) of a decoded clip; CLIP_SHAPE at the default."""
    return (check_clip_length(clip_length),) + CLIP_SHAPE[1:]
# output sampling for numerics checks of a served run (bench.py): the loader
# tags every CHECK_EVERY-th video with its decode source, and a final-step
# runner with RNB_CHECK_DIR set writes those videos' logits there
CHECK_EVERY = int(os.environ.get("RNB_CHECK_EVERY", "13"))
# 15-clip videos are 1 in 11: tag more of them so every check covers them
CHECK_EVERY_LARGE = int(os.environ.get("RNB_CHECK_EVERY_LARGE", "3"))
CHECK_MAX = int(os.environ.get("RNB_CHECK_MAX", "6"))         # per stratum and process
DEFAULT_DTYPE = "fp32"       # the reference computes in fp32 (model.py:149,225)


def _dtype(d):
    from .engine import _as_dtype
    return _as_dtype(d if d is not None else DEFAULT_DTYPE)


def default_bn_mode(bn_mode, dtype, arch=None) -> str:
    """BatchNorm numerics of the runner plugins when a config does not say.
    The reference never calls ``.eval()`` (its runner only wraps the forward
    in ``torch.no_grad()``, reference runner.py:45), so every BatchNorm
    normalises with the statistics of the video being served: 'batch'
    (per-video segments, graphed at fp32). bf16 batch BN runs eagerly, so
    bf16 defaults to the folded 'eval' numerics. Configs choose either with
    ``"bn_mode"`` (per step or in ``defaults``). ``arch="torchvision"``
    defaults to 'eval' at both dtypes: published weights are served on their
    running statistics ('batch' stays available, graphed at fp32)."""
    if bn_mode is None:
        if check_arch(arch) == "torchvision":
            return "eval"
        return "batch" if _dtype(dtype) == torch.float32 else "eval"
    if bn_mode not in ("eval", "batch"):
        raise ValueError("bn_mode must be 'eval' or 'batch', got %r" % (bn_mode,))
    return bn_mode


def clip_channels(dtype) -> int:
    """Channels of a decoded NDHWC clip pixel (RGB padded to 16 bytes)."""
    from ...ops.video import IN_CHANNELS_P, IN_CHANNELS_P_F32
    return IN_CHANNELS_P_F32 if _dtype(dtype) == torch.float32 else IN_CHANNELS_P


def _resolve_backend(backend: str, device: torch.device) -> str:
    if backend == "auto":
        return "hip" if device.type == "cuda" else "torch"
    if backend == "hip" and device.type != "cuda":
        raise ValueError("backend 'hip' needs a GPU device, got %s" % device)
    return backend


def build_network(start_index: int, end_index: int, num_classes: int = 400,
                  layer_sizes=None, depth: Optional[int] = None, seed: int = 0,
                  ckpt_path: Optional[str] = None, arch: Optional[str] = None,
                  midplanes: Optional[str] = None, bn_eps: Optional[float] = None):
    """The module tree of layers [start_index, end_index], seeded at random or
    loaded from ``ckpt_path``. ``arch="reference"`` (default): the reference's
    tree and checkpoint format. ``arch="torchvision"``: torchvision's
    ``VideoResNet`` layout (``r2plus1d_18``, IG65M ``r2plus1d_34``); the
    mid-channel counts come from the checkpoint's tensor shapes when there is
    one, else from ``midplanes`` ("block", torchvision's rule, or "conv");
    ``bn_eps`` is the BatchNorms' eps (a state dict does not carry it)."""
    arch = check_arch(arch)
    midplanes, bn_eps = check_midplanes(midplanes), check_bn_eps(bn_eps)
    sizes = normalize_layer_sizes(start_index, end_index, layer_sizes, depth)
    if arch == "reference":
        if midplanes is not None or bn_eps is not None:
            raise ValueError("midplanes / bn_eps belong to arch='torchvision'")
        net = R2Plus1DLayerWrapper(start_index, end_index, num_classes, sizes)
        init_random_(net, seed)
        if ckpt_path:
            ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=True)
            state = ckpt.get("state_dict", ckpt) if isinstance(ckpt, dict) else ckpt
            load_reference_state_dict(net, state)
        return net.eval()
    state = None
    if ckpt_path:
        ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=True)
        state = ckpt.get("state_dict", ckpt) if isinstance(ckpt, dict) else ckpt
    net = TVVideoResNet(start_index, end_index, num_classes, sizes,
                        midplanes=midplanes or "block",
                        bn_eps=DEFAULT_BN_EPS if bn_eps is None else bn_eps,
                        mids=tv_state_mids(state) if isinstance(state, dict) else None)
    init_random_(net, seed)
    if state is not None:
        load_torchvision_state_dict(net, state)
    return net.eval()


def build_engine(device: torch.device, start_index=1, end_index=5, num_classes=400,
                 layer_sizes=None, depth=None, backend="auto", bn_mode="eval", seed=0,
                 ckpt_path=None, max_clips=DEFAULT_MAX_CLIPS, use_graphs=True,
                 autotune=True, dtype=None, buckets=None,
                 clip_length=DEFAULT_CLIP_LENGTH, arch=None, midplanes=None, bn_eps=None):
    clip_length = check_clip_length(clip_length)
    arch = check_arch(arch)
    backend = _resolve_backend(backend, device)
    if backend == "hip":
        # before any weight is built: a call of max_clips clips must fit the
        # kernels' per-launch limits at this clip length
        check_max_clips(max_clips, start_index, end_index, _dtype(dtype), clip_length, arch)
    net = build_network(start_index, end_index, num_classes, layer_sizes, depth, seed,
                        ckpt_path, arch, midplanes, bn_eps)
    eng = R2P1DEngine(net, device, backend=backend, bn_mode=bn_mode, dtype=_dtype(dtype),
                      clip_length=clip_length)
    # batch-statistics BN is graphed for fp32 (per-video segments from a
    # static offsets tensor); bf16 batch BN runs eagerly
    if backend == "hip" and use_graphs and (bn_mode == "eval" or _dtype(dtype) == torch.float32):
        kw = {} if buckets is None else {"buckets": buckets}
        return GraphedEngine(eng, max_clips, autotune=autotune, **kw)
    return eng


def _to_boundary(x: torch.Tensor, start_index: int, dtype=torch.float32,
                 clip_length=DEFAULT_CLIP_LENGTH) -> torch.Tensor:
    """Accept the reference NCDHW fp32 layout as well as the NDHWC boundary
    (the frame count is the tensor's own: both layouts carry it)."""
    cp = boundary_channels_p(start_index, dtype)
    if x.dim() == 5 and x.shape[-1] == cp and x.shape[1] != LAYER_INPUT_CTHW[start_index][0]:
        return x.to(dtype).contiguous()
    c = LAYER_INPUT_CTHW[start_index][0]
    if x.dim() == 5 and x.shape[1] == c:
        from ...ops.video import ncdhw_to_ndhwc
        return ncdhw_to_ndhwc(x, cp, dtype=dtype)
    raise ValueError("unexpected input of shape %s for layer %d" % (tuple(x.shape),
                                                                     start_index))


class R2P1DRunner(RunnerModel):
    """Layers [start_index, end_index] of R(2+1)D (1-indexed, inclusive)."""

    def __init__(self, device, start_index=1, end_index=5, num_classes=400,
                 layer_sizes=None, depth=None, block_type=None, backend="auto",
                 bn_mode=None, seed=0, ckpt_path=None, max_clips=DEFAULT_MAX_CLIPS,
                 warmup=3, use_graphs=True, autotune=True, dtype=None,
                 max_batch_videos=1, batch_wait_ms=0.0, bucket_step=None, lanes=1,
                 stream_priority=0, clip_length=DEFAULT_CLIP_LENGTH, arch=None,
                 midplanes=None, bn_eps=None, **unused):
        super().__init__(device)
        self.clip_length = clip_length = check_clip_length(clip_length)
        self.arch = arch = check_arch(arch)
        midplanes, bn_eps = check_midplanes(midplanes), check_bn_eps(bn_eps)
        if start_index < 1:
            raise ValueError("Wrong layer index for the starting layer! The start_index "
                             "(%d) should be more than or equal to 1." % start_index)
        if end_index > 5:
            raise ValueError("Wrong layer index for the ending layer! The end_index (%d) "
                             "should be less than or equal to 5." % end_index)
        self.start_index, self.end_index = start_index, end_index
        self.max_clips = int(max_clips)
        self.dtype = _dtype(dtype)
        self.bn_mode = bn_mode = default_bn_mode(bn_mode, self.dtype, arch)
        self.max_batch_videos = int(max_batch_videos)
        self.batch_wait_s = float(batch_wait_ms) / 1000.0
        # "geo": geometric spacing + bucket-aligned gathering (gather_fit)
        buckets = parse_bucket_step(bucket_step, self.max_clips)
        self.engine = build_engine(device, start_index, end_index, num_classes,
                                   layer_sizes, depth, backend, bn_mode, seed, ckpt_path,
                                   self.max_clips, use_graphs, autotune, self.dtype, buckets,
                                   clip_length, arch, midplanes, bn_eps)
        # lanes > 1: that many graphed engines (own weights copy, BN buffers and
        # graph pool each; the same seed / checkpoint, so identical outputs) on
        # their own streams, calls rotating over them. One-video calls leave
        # most of the chip idle and are ~220 short dispatches: two in flight on
        # two streams overlap (scripts/lanes_probe.py: 1-clip calls 2.28 ->
        # 1.33 ms each, 16-clip 6.87 -> 5.69 ms; profiles/r4_lanes_probe.txt).
        # Each lane keeps its own BatchNorm running statistics.
        self.lanes = max(1, int(lanes)) if (isinstance(self.engine, GraphedEngine)
                                             and device.type == "cuda") else 1
        self._lane_engines = [self.engine]
        for _ in range(self.lanes - 1):
            self._lane_engines.append(build_engine(
                device, start_index, end_index, num_classes, layer_sizes, depth, backend,
                bn_mode, seed, ckpt_path, self.max_clips, use_graphs, autotune, self.dtype,
                buckets, clip_length, arch, midplanes, bn_eps))
        # lane streams at DEFAULT priority, not the runner's (runner.py passes
        # the queue group's, e.g. the high-priority 15-clip replica's): the
        # round-4 advice asked for the runner's; measured interleaved, it costs
        # 11 % of the headline and raises the mi = 10 p99 (1394 vs 1562
        # videos/s, p99 15.2 vs 10.7 ms: profiles/r5_ab_lane_priority_guard.txt)
        # -- a high-priority queue holding 60 % of the clips (15-clip videos)
        # starves the small replicas' dispatches instead of overlapping them.
        # RNB_LANE_PRIORITY=runner restores the runner's priority.
        lane_prio = os.environ.get("RNB_LANE_PRIORITY", "0")
        lane_prio = int(stream_priority) if lane_prio == "runner" else int(lane_prio)
        self.lane_stream_priority = lane_prio
        self._lane_streams = ([torch.cuda.Stream(device, priority=lane_prio)
                               for _ in range(self.lanes)] if self.lanes > 1 else None)
        self._lane_done = [None] * self.lanes     # completion event of each lane's last call
        self._lane = 0                             # lane of the next call
        self.last_event = None                     # completion event of the last call
        for eng in self._lane_engines:
            if isinstance(eng, GraphedEngine):
                eng.prepare()
            if device.type == "cuda" and os.environ.get("RNB_REPORT_MEMORY") == "1":
                print("[runner gpu %d] %d graph buckets, capture %.1f s, %.1f GB allocated, "
                      "%.1f GB reserved" % (device.index or 0, len(self.engine.graphs),
                                            self.engine.capture_s,
                                            torch.cuda.memory_allocated(device) / 2 ** 30,
                                            torch.cuda.memory_reserved(device) / 2 ** 30),
                      flush=True)
        n = min(10, self.max_clips)
        tmp = torch.randn(boundary_shape(start_index, n, self.dtype, clip_length)
                          ).to(self.dtype).to(device)
        for _ in range(warmup):
            self.engine(tmp)
        if device.type == "cuda":
            torch.cuda.current_stream(device).synchronize()
        for eng in self._lane_engines:
            if getattr(eng, "range_guard", None) is not None:
                eng.range_guard.reset()
        self._gather_ptr = None
        self._gather_buf = None
        self._check_dir = os.environ.get("RNB_CHECK_DIR") or None
        self._checked = {}               # samples written per stratum
        # h3 range guard (ops/conv_f32.RangeGuard): graphed calls are checked
        # when the runner sees them complete (on_complete), in call order. An
        # engine whose convs picked no h3 config (RNB_H3=0, full-range picks)
        # cannot trip it: then a non-final stage need not synchronise each
        # call before publishing (runner.py)
        self.range_guarded = any(
            getattr(e, "range_guard", None) is not None
            and (not callable(getattr(e, "uses_h3", None)) or e.uses_h3())
            for e in self._lane_engines)
        self._guard_calls = []           # (graphed engine, output, call record) in flight
        self.range_fallbacks = 0
        self._direct_calls = self._staged_calls = 0     # intermediate-stage outputs

    def on_complete(self, outputs) -> None:
        """runner.py: the oldest call in flight has completed. If an h3 conv of
        it produced a non-finite value (an input past the fp16 range of the h3
        split), recompute its output on full-range kernels before it is used."""
        if not self._guard_calls:
            return
        eng, out, call = self._guard_calls.pop(0)
        if eng.range_fallback(out, call):
            self.range_fallbacks += 1
            print("[runner] h3 range guard: call of %d rows re-run on full-range kernels "
                  "(%d so far)" % (out.shape[0], self.range_fallbacks), flush=True)

    def runtime_stats(self) -> dict:
        st = {"h3_range_fallbacks": self.range_fallbacks} if self.range_guarded else {}
        # conv shapes this process timed vs took from the tuning cache / seed
        # table (ops/tuning.py): a replica that starts after another has tuned
        # the same shapes should time none of them
        from ...ops import tuning
        ts = tuning.stats()
        st.update({"tune_tuned": ts["tuned"], "tune_read": ts["read"],
                   "tune_runners_tuning": int(ts["tuned"] > 0), "tune_runners": 1})
        if self.end_index < 5:
            st.update(direct_slot_calls=self._direct_calls, staged_slot_calls=self._staged_calls)
        return st

    def call_into(self, tensors, non_tensors, time_card, out):
        """Intermediate stage (end_index < 5; runner.py direct_out): write the
        boundary activation straight into the output slot ``out[0]``. The
        fp32 batch-BN graphs end in a BatchNorm apply that writes through a
        device-held pointer, so the replay targets the slot itself and no
        staging copy runs (the reference copies each output
        into its slot, runner.py:156-173). Other engines compute into their
        own buffer and copy the rows into the slot."""
        x = tensors[0]
        eng = self.engine
        slot = out[0]
        if (self.lanes == 1 and isinstance(eng, GraphedEngine) and eng.indirect_out
                and x.shape[0] > 0 and self._gather_ptr is not None
                and x.data_ptr() == self._gather_ptr):
            self._gather_ptr = None
            offs = self._clip_offsets(time_card, x.shape[0])
            y = eng.replay(x.shape[0], clip_offsets=offs, out=slot)
            if eng.range_guard is not None:
                self._guard_calls.append((eng, y, eng.last_call))
            self._direct_calls += 1
            return (y,), non_tensors, time_card
        (y,), nts, tc = self._call(tensors, non_tensors, time_card)
        if self.lanes > 1 and self.last_event is not None:
            torch.cuda.current_stream(self.device).wait_event(self.last_event)
        if y.shape[0]:
            slot[:y.shape[0]].copy_(y)
        if self._guard_calls and self._guard_calls[-1][1] is y:
            # a guard re-run of this call must land in the slot
            e, _, call = self._guard_calls[-1]
            self._guard_calls[-1] = (e, slot[:y.shape[0]], call)
        self._staged_calls += 1
        return (slot[:y.shape[0]],), nts, tc

    # consumer-side batching (runner.py): up to max_batch_videos queued
    # videos per call, their rows pulled into the graph's static input
    def gather_limits(self):
        if self.max_batch_videos <= 1 and not isinstance(self.engine, GraphedEngine):
            return None
        return (max(1, self.max_batch_videos), self.max_clips, self.batch_wait_s)

    # trim a gathered call to a bucket boundary when padding up to the next
    # bucket would add more than this fraction of rows (runner.py gather;
    # RNB_FIT_PAD_FRAC overrides, >= 1 never trims)
    FIT_PAD_FRAC = float(os.environ.get("RNB_FIT_PAD_FRAC", "0.03"))

    def gather_fit(self, rows: int) -> int:
        """Rows a gathered call of ``rows`` should keep: ``rows`` when padding
        to its graph bucket is cheap, else the largest bucket below (runner.py
        defers the trailing items to the next call)."""
        eng = self.engine
        if not isinstance(eng, GraphedEngine) or rows <= 1:
            return rows
        up = eng.bucket_for(rows)
        if up - rows <= self.FIT_PAD_FRAC * rows:
            return rows
        return eng.bucket_floor(rows) or rows

    def completion_event(self):
        """lanes > 1: the event that completes the last call (it ran on a lane
        stream, not on the runner's); None otherwise."""
        return self.last_event if self.lanes > 1 else None

    def inflight_calls(self) -> int:
        """Calls the final-step runner should keep in flight (runner.py)."""
        return self.lanes - 1

    def gather_buffers(self, rows: int):
        if self.lanes > 1:
            ev = self._lane_done[self._lane]
            if ev is not None:
                # the lane's previous call must be done reading its static input
                torch.cuda.current_stream(self.device).wait_event(ev)
        eng = self._lane_engines[self._lane]
        if isinstance(eng, GraphedEngine) and rows > 0:
            static_in, _ = eng.input_buffer(rows)
        else:
            if self._gather_buf is None:
                self._gather_buf = torch.empty(
                    boundary_shape(self.start_index, self.max_clips, self.dtype,
                                   self.clip_length),
                    dtype=self.dtype, device=self.device)
            static_in = self._gather_buf
        self._gather_ptr = static_in.data_ptr()
        return (static_in,)

    def input_shape(self):
        return (boundary_shape(self.start_index, self.max_clips, self.dtype,
                               self.clip_length),)

    @staticmethod
    def output_shape():
        return ((DEFAULT_MAX_CLIPS, 400),)

    @classmethod
    def output_shape_for(cls, start_index=1, end_index=5, num_classes=400,
                         max_clips=DEFAULT_MAX_CLIPS, dtype=None,
                         clip_length=DEFAULT_CLIP_LENGTH, **kwargs):
        clip_length = check_clip_length(clip_length)
        if end_index == 5:
            return ((max_clips, num_classes),)
        return (boundary_shape(end_index + 1, max_clips, _dtype(dtype), clip_length),)

    @classmethod
    def output_dtypes_for(cls, end_index=5, dtype=None, **kwargs):
        return (torch.float32,) if end_index == 5 else (_dtype(dtype),)

    @staticmethod
    def _clip_offsets(time_card, n: int):
        """Clip ranges of the BN segments of this call (bn_mode='batch'); None =
        one segment. A segment is one queued item as the reference would run
        it: a single video keeps its own statistics, while a Batcher batch
        (reference batcher.py:28 + runner.py:125-126: one forward over the
        concatenated videos) is normalised with its joint statistics."""
        if not isinstance(time_card, TimeCardList) or n == 0:
            return None
        rows = getattr(time_card, "item_rows", None)
        if not rows or len(rows) < 2:
            return None
        offs = [0]
        for r in rows:
            if int(r) > 0:             # empty segments (0-row items) add no BN segment
                offs.append(offs[-1] + int(r))
        if offs[-1] != n or len(offs) < 3:
            return None
        return offs

    def _keep_samples(self, y: torch.Tensor, time_card) -> None:
        """RNB_CHECK_DIR: write the logits of tagged videos (loader
        ``clip_src``) of this call, at most CHECK_MAX per runner, for an
        offline recomputation (bench.py ``numerics``)."""
        cards = time_card.time_cards if isinstance(time_card, TimeCardList) else [time_card]
        rows = (list(time_card.item_rows) if isinstance(time_card, TimeCardList)
                and getattr(time_card, "item_rows", None) else [y.shape[0]])
        if len(rows) != len(cards):
            return                     # Batcher items: several videos per segment
        from ...numerics import stratum_of, write_sample
        off, call_rows = 0, int(y.shape[0])
        for tc, n in zip(cards, rows):
            src = tc.extra.get("clip_src")
            if src is not None and n == len(src[1]) and n and tc.sub_id is None:
                stratum = stratum_of("runner", n, call_rows)
                if self._checked.get(stratum, 0) < CHECK_MAX:
                    self._checked[stratum] = self._checked.get(stratum, 0) + 1
                    if self.lanes > 1:          # y was written on a lane stream
                        torch.cuda.current_stream(self.device).wait_event(self.last_event)
                    write_sample(self._check_dir, tc.id, "runner", src[0], src[1],
                                 y[off:off + n].float().cpu().numpy(), self.bn_mode,
                                 str(self.dtype), call_rows=call_rows,
                                 clip_length=self.clip_length,
                                 step=tc.extra.get("clip_step", (1, 1)))
            off += n

    def __call__(self, tensors, non_tensors, time_card):
        out = self._call(tensors, non_tensors, time_card)
        if self._check_dir and self.end_index == 5 and time_card is not None:
            self._keep_samples(out[0][0], time_card)
        return out

    def _call(self, tensors, non_tensors, time_card):
        if self.lanes == 1:
            return (self._run(self.engine, tensors[0], time_card),), non_tensors, time_card
        lane = self._lane
        self._lane = (lane + 1) % self.lanes
        cur = torch.cuda.current_stream(self.device)
        ls = self._lane_streams[lane]
        ls.wait_stream(cur)                        # the input rows were pulled on `cur`
        with torch.cuda.stream(ls):
            y = self._run(self._lane_engines[lane], tensors[0], time_card)
            ev = torch.cuda.Event()
            ev.record(ls)
        self._lane_done[lane] = ev
        self.last_event = ev
        return (y,), non_tensors, time_card

    def _run(self, eng, x, time_card):
        offs = (self._clip_offsets(time_card, x.shape[0]) if self.bn_mode == "batch"
                else None)
        if (self._gather_ptr is not None and x.data_ptr() == self._gather_ptr
                and isinstance(eng, GraphedEngine) and x.shape[0] > 0):
            # rows already sit in the bucket graph's static input: replay only
            self._gather_ptr = None
            y = eng.replay(x.shape[0], clip_offsets=offs)
            if eng.range_guard is not None:
                self._guard_calls.append((eng, y, eng.last_call))
            return y
        self._gather_ptr = None
        x = _to_boundary(x, self.start_index, self.dtype, self.clip_length)
        if isinstance(eng, GraphedEngine) and x.shape[0] > 0:
            y = eng.forward(x, clip_offsets=offs) if self.bn_mode == "batch" else eng(x)
            if eng.range_guard is not None:
                self._guard_calls.append((eng, y, eng.last_call))
            return y
        if getattr(eng, "range_guard", None) is not None and x.shape[0] > 0:
            # eager hip engine: checked right here (waits for the call)
            before = eng.range_guard.fallbacks
            y = eng.forward_checked(x, clip_offsets=offs)
            self.range_fallbacks += eng.range_guard.fallbacks - before
            return y
        if self.bn_mode == "batch" and x.shape[0] > 0:
            return eng.forward(x, clip_offsets=offs)
        return eng(x)


class R2P1DVideoPathIterator(VideoPathIterator):
    """Kinetics-style ``root/label/video`` walk when ``root`` (or env
    ``RNB_VIDEO_ROOT``) exists; endless synthetic paths otherwise."""

    def __init__(self, root: Optional[str] = None, seed: int = 0):
        root = root or os.environ.get("RNB_VIDEO_ROOT")
        if root and os.path.isdir(root):
            self._it = DirectoryVideoPathIterator(root)
        else:
            self._it = SyntheticVideoPathIterator(seed=seed)

    def __iter__(self):
        return iter(self._it)


def _decoder_args(decoder_args, crop, filter):
    """``decoder_args`` with the step-level ``crop`` / ``filter`` kwargs (what a
    config's ``defaults`` or ``--set`` reach) laid over it."""
    args = dict(decoder_args or {})
    if crop is not None:
        args["crop"] = crop
    if filter is not None:
        args["filter"] = filter
    return args or None


def expand_views(starts, views: int):
    """Clip starts -> (start, view) of every output row, the views of a clip
    adjacent: the row order of ``decode`` with ``views`` views per clip."""
    return [s for s in starts for _ in range(views)], [v for _ in starts for v in range(views)]


class R2P1DLoader(RunnerModel):
    """Video path -> sampled clips, NDHWC [n, clip_length, 112, 112, C] (fp32 C=4,
    bf16 C=8; clip_length 8, 16 or 32 frames, default 8).

    A decoder with ``views`` > 1 (``decoder_args`` / ``crop`` of
    ``{"short_side": S, "views": 3}``) returns that many rows per temporal
    clip: the loader keeps ``min(len(starts), max_clips // views)`` clips, emits
    ``views`` rows for each and counts rows in ``time_card.num_clips``, so
    slots, buckets and the aggregator (which sums every row of a video) are
    sized by ``max_clips`` as before. ``crop`` and ``filter`` are shorthands
    for the same keys of ``decoder_args``.

    ``labels="dir"``: the class index of a ``root/<name>/<video>`` path
    (``DirectoryLabels``: ``<name>``'s position among ``root``'s sorted
    sub-directories, or its line in ``class_names=FILE``) travels in
    ``time_card.extra["label"]`` to the aggregator, which counts top-1 / top-k
    hits by it; synthetic paths get none.

    ``frame_step`` (an integer >= 1) or ``fps`` (a positive number or
    ``"n:d"``; not both) sets the step ``(p, q)`` clips are taken at
    (``sampler.clip_frames``): every ``frame_step``-th frame, or the exact
    ``source_fps / fps`` of each file, whose rate the decoder knows
    (``source_fps_of``: a Y4M header's ``F`` field, else the decoder's
    ``source_fps`` argument; a file without one raises). The sampler fits
    clips by the span they cover, every ``decode`` gets the step, and a tagged
    request carries it in ``time_card.extra["clip_step"]`` when it is not
    ``(1, 1)``. ``placement="uniform"`` centres the clips instead of drawing
    their offset (``R2P1DSampler``)."""

    # decode kernels are tiny and gate the consumers: run them on a
    # high-priority HIP stream so they do not queue behind the conv kernels
    stream_priority = -1

    def __init__(self, device, num_clips_population=(1, 15), num_clips_weights=(10, 1),
                 decoder="synthetic", seed=None, max_clips=DEFAULT_MAX_CLIPS,
                 warmup=3, dtype=None, decoder_args=None,
                 clip_length=DEFAULT_CLIP_LENGTH, crop=None, filter=None, labels=None,
                 class_names=None, frame_step=1, fps=None, placement="random", **unused):
        super().__init__(device)
        try:
            self.frame_step = check_frame_step(frame_step)
            self.fps = parse_rate(fps, "fps")
            if self.fps is not None and self.frame_step != 1:
                raise ValueError("frame_step = %r and fps = %r: give one of them"
                                 % (frame_step, fps))
            if placement not in PLACEMENTS:
                raise ValueError("placement = %r, expected one of %s"
                                 % (placement, PLACEMENTS))
        except ValueError as err:
            raise ValueError("R2P1DLoader: %s" % err)
        if labels not in (None, "dir"):
            raise ValueError("R2P1DLoader: labels = %r, expected None or \"dir\"" % (labels,))
        if class_names is not None and labels is None:
            raise ValueError("R2P1DLoader: class_names = %r needs labels = \"dir\""
                             % (class_names,))
        self.labels = DirectoryLabels(class_names) if labels == "dir" else None
        self.clip_length = check_clip_length(clip_length)
        self.sampler = R2P1DSampler(clip_length=self.clip_length,
                                    num_clips_population=num_clips_population,
                                    num_clips_weights=num_clips_weights, seed=seed,
                                    placement=placement)
        self.dtype = _dtype(dtype)
        self.decoder = make_decoder(decoder, device, *clip_shape(self.clip_length),
                                    dtype=self.dtype,
                                    decoder_args=_decoder_args(decoder_args, crop, filter))
        self.max_clips = max_clips
        self.views = int(getattr(self.decoder, "views", 1))
        if int(max_clips) < self.views:
            raise ValueError("R2P1DLoader: max_clips = %r holds no clip of %d views (the "
                             "decoder's crop 'views'); max_clips must be >= views"
                             % (max_clips, self.views))
        self.decoder.warmup(warmup)
        if device.type == "cuda":
            torch.cuda.current_stream(device).synchronize()

    def _step_of(self, vid: int, path: str):
        """The step (p, q) the clips of a probed file are taken at."""
        if self.fps is None:
            return self.frame_step, 1
        source = self.decoder.source_fps_of(vid)
        if source is None:
            raise ValueError("%s: fps = %s needs the file's frame rate, and it has none (a Y4M "
                             "header's field 'F', or the decoder argument 'source_fps')"
                             % (path, self.fps))
        return step_of(fps=self.fps, source_fps=source)

    def place(self, path: str):
        """(video id, clip start frames, step) of ``path``: the probe, the
        file's step and one draw of the sampler for clips of that span."""
        vid, length = self.decoder.probe(path)
        step = self._step_of(vid, path)
        starts = self.sampler.sample(length, span=clip_span(self.clip_length, step))
        return vid, (starts or [])[:self.max_clips // self.views], step

    def _sample(self, path: str, time_card=None):
        """(video id, clip start frames, step) of ``path``; tags sampled requests
        with what a numerics check needs to decode the same clips again."""
        vid, starts, step = self.place(path)
        if time_card is not None and self.labels is not None:
            label = self.labels.label(path)
            if label is not None:
                time_card.extra["label"] = label
        if time_card is not None and (time_card.id % CHECK_EVERY == 0 or (
                len(starts) >= 15 and time_card.id % CHECK_EVERY_LARGE == 0)):
            # one start per output row, so that the sample files keep
            # len(starts) == logits rows
            time_card.extra["clip_src"] = (int(vid), [int(s) for s in
                                                      expand_views(starts, self.views)[0]])
            if step != (1, 1):
                time_card.extra["clip_step"] = step
        return vid, starts, step

    def load(self, path: str, out: Optional[torch.Tensor] = None, time_card=None):
        vid, starts, step = self._sample(path, time_card)
        return self.decoder.decode(vid, starts, out=None if out is None else
                                   out[:len(starts) * self.views], step=step)

    def __call__(self, tensors, non_tensors, time_card):
        frames = self.load(non_tensors, time_card=time_card)
        time_card.num_clips = int(frames.shape[0])
        return (frames,), None, time_card

    def call_into(self, tensors, non_tensors, time_card, out):
        """Decode straight into the output slot ``out[0]`` (runner.py direct_out:
        no staging tensor, no slot copy)."""
        frames = self.load(non_tensors, out=out[0], time_card=time_card)
        time_card.num_clips = int(frames.shape[0])
        return (frames,), None, time_card

    def call_into_segments(self, tensors, non_tensors, time_card, outs):
        """Segment-parallel producer (``num_segments`` = len(outs)): decode
        each segment's clips (the reference's row split, runner.py:149-151)
        straight into its own output slot ``outs[k][0]``; returns the rows per
        segment (runner.py direct_seg: no staging tensor, no slot copy;
        SURVEY.md K31). The synthetic decoder renders a clip from (video,
        start frame) only, so the segments equal the split of one decode."""
        from ...control import segment_bounds
        vid, starts, step = self._sample(non_tensors, time_card)
        if self.views > 1:      # the rows are split, not the clips: a segment names its views
            row_starts, row_views = expand_views(starts, self.views)
        rows = []
        for k, out in enumerate(outs):
            a, b = segment_bounds(len(starts) * self.views, len(outs), k)
            if b > a and self.views > 1:
                self.decoder.decode(vid, row_starts[a:b], out=out[0][:b - a],
                                    views=row_views[a:b], step=step)
            elif b > a:
                self.decoder.decode(vid, starts[a:b], out=out[0][:b - a], step=step)
            rows.append(b - a)
        time_card.num_clips = len(starts) * self.views
        return rows, None, time_card

    def input_shape(self):
        return None

    @staticmethod
    def output_shape():
        return ((DEFAULT_MAX_CLIPS,) + CLIP_SHAPE + (clip_channels(None),),)

    @classmethod
    def output_shape_for(cls, max_clips=DEFAULT_MAX_CLIPS, dtype=None,
                         clip_length=DEFAULT_CLIP_LENGTH, **kwargs):
        return ((max_clips,) + clip_shape(clip_length) + (clip_channels(dtype),),)

    @classmethod
    def output_dtypes_for(cls, dtype=None, **kwargs):
        return (_dtype(dtype),)


class R2P1DSingleStep(RunnerModel):
    """Loader + whole R(2+1)D in one stage, no pipelining (model.py:161-235)."""

    def __init__(self, device, num_classes=400, layer_sizes=None, depth=None,
                 block_type=None, num_clips_population=(1, 15), num_clips_weights=(10, 1),
                 decoder="synthetic", seed=None, model_seed=0, backend="auto",
                 bn_mode=None, ckpt_path=None, max_clips=DEFAULT_MAX_CLIPS, warmup=3,
                 use_graphs=True, autotune=True, dtype=None, decoder_args=None,
                 clip_length=DEFAULT_CLIP_LENGTH, crop=None, filter=None, frame_step=1,
                 fps=None, placement="random", arch=None, midplanes=None, bn_eps=None,
                 **unused):
        super().__init__(device)
        clip_length = check_clip_length(clip_length)
        self.loader = R2P1DLoader(device, num_clips_population, num_clips_weights,
                                  decoder=decoder, seed=seed, max_clips=max_clips,
                                  warmup=warmup, dtype=dtype, decoder_args=decoder_args,
                                  clip_length=clip_length, crop=crop, filter=filter,
                                  frame_step=frame_step, fps=fps, placement=placement)
        self.runner = R2P1DRunner(device, 1, 5, num_classes,
                                  layer_sizes=layer_sizes, depth=depth, backend=backend,
                                  bn_mode=bn_mode, seed=model_seed, ckpt_path=ckpt_path,
                                  max_clips=max_clips, warmup=warmup,
                                  use_graphs=use_graphs, autotune=autotune, dtype=dtype,
                                  clip_length=clip_length, arch=arch, midplanes=midplanes,
                                  bn_eps=bn_eps)

    @property
    def range_guarded(self) -> bool:
        return self.runner.range_guarded

    def on_complete(self, outputs) -> None:
        self.runner.on_complete(outputs)

    def runtime_stats(self) -> dict:
        return self.runner.runtime_stats()

    def __call__(self, tensors, non_tensors, time_card):
        eng = self.runner.engine
        if isinstance(eng, GraphedEngine) and self.runner.device.type == "cuda":
            # decode straight into the bucket graph's input buffer
            vid, starts, step = self.loader.place(non_tensors)
            nrows = len(starts) * self.loader.views
            time_card.num_clips = nrows
            if starts:
                static_in, _ = eng.input_buffer(nrows)
                self.loader.decoder.decode(vid, starts, out=static_in[:nrows], step=step)
                y = eng.replay(nrows)
                if eng.range_guard is not None:
                    self.runner._guard_calls.append((eng, y))
                return (y,), None, time_card
            frames = self.loader.decoder.empty()
            (logits,), _, _ = self.runner((frames,), None, time_card)
            return (logits,), None, time_card
        frames = self.loader.load(non_tensors)
        time_card.num_clips = int(frames.shape[0])
        (logits,), _, _ = self.runner((frames,), None, time_card)
        return (logits,), None, time_card

    def input_shape(self):
        return None

    @staticmethod
    def output_shape():
        return ((DEFAULT_MAX_CLIPS, 400),)

    @classmethod
    def output_shape_for(cls, num_classes=400, max_clips=DEFAULT_MAX_CLIPS, **kwargs):
        return ((max_clips, num_classes),)


class R2P1DAggregator(RunnerModel):
    """Sums clip logits per video; re-joins ``aggregate`` segments by id.

    Accepts a single request's rows or a batch (``TimeCardList``, e.g. from a
    batching runner upstream): a batch is split per request by the rows each
    one brought (``extra["rows"]``, set by the gathering runner) or, for whole
    videos, by their clip counts. Segments of one video may arrive in
    different batches; a video is emitted once all ``aggregate`` segments
    arrived (reference model.py:238-285, with batching added).

    ``scores`` / ``top_k`` (ops/video.video_scores: "logit_sum", "logit_mean",
    "softmax_sum", "softmax_mean"; 1 <= top_k <= 16): with the defaults
    ("logit_sum", 1) a video's output is the argmax of its summed logits, an
    int, computed on the host as the reference does. Otherwise one
    ``video_scores`` launch per call scores every video of the call on the
    tensor's device (the torch mirror on a CPU device), only the [videos][k]
    results cross to the host, and a video's output is ``(classes, scores)``,
    two k-tuples, best first. With ``aggregate`` > 1 a segment contributes its
    "_sum" scores and its row count; the last one to arrive takes the top-k of
    the total (divided by the total row count for the "_mean" kinds).

    A time card with ``extra["label"]`` (R2P1DLoader ``labels``) is counted in
    every mode: ``runtime_stats()`` returns ``eval_videos``, ``eval_top1`` and
    ``eval_top<k>``. ``results_path``: one JSON line per emitted video (id,
    label, classes, scores) appended to ``<results_path>.<pid>.jsonl``."""

    def __init__(self, device, aggregate=1, clip_length=DEFAULT_CLIP_LENGTH,
                 scores="logit_sum", top_k=1, results_path=None, **unused):
        super().__init__(device)
        # sizes nothing by it (logit rows only); checked so that a pipeline's
        # "defaults" value is validated at every step
        self.clip_length = check_clip_length(clip_length)
        self.aggregate = int(aggregate)
        self.results = {}
        self._check_dir = os.environ.get("RNB_CHECK_DIR") or None
        self._checked = 0
        self.scores, self.top_k = str(scores), int(top_k)
        vops.check_score_args(self.scores, self.top_k)
        self._scored = (self.scores, self.top_k) != ("logit_sum", 1)
        self.results_path = results_path or None
        self._results_file = None
        self.eval_videos = self.eval_top1 = self.eval_topk = 0

    def _sum(self, tensor) -> np.ndarray:
        return tensor.detach().float().cpu().numpy().sum(axis=0)

    def runtime_stats(self) -> dict:
        if self._results_file is not None:
            self._results_file.flush()
        if not self.eval_videos:
            return {}
        st = {"eval_videos": self.eval_videos, "eval_top1": self.eval_top1}
        st["eval_top%d" % self.top_k] = self.eval_topk
        return st

    def _tracks(self, tc) -> bool:
        return self.results_path is not None or "label" in tc.extra

    def _emit(self, tc, classes, scores) -> None:
        """Count one finished video against its label; log it to results_path."""
        label = tc.extra.get("label")
        if label is not None:
            self.eval_videos += 1
            self.eval_top1 += int(classes[0] == label)
            self.eval_topk += int(label in classes)
        if self.results_path is not None:
            if self._results_file is None:
                self._results_file = open("%s.%d.jsonl" % (self.results_path, os.getpid()), "a")
            self._results_file.write(json.dumps(
                {"id": int(tc.id), "label": None if label is None else int(label),
                 "classes": [int(c) for c in classes],
                 "scores": [float(s) for s in scores]}) + "\n")
            self._results_file.flush()

    @staticmethod
    def _card_rows(tc) -> int:
        n = tc.extra.get("rows")
        if n is None:
            n = tc.num_clips if tc.num_clips is not None else 1
        return n

    def _top(self, rows, offs, kind):
        """One video_scores launch over ``rows``; the [videos][k] results on the host."""
        off = torch.tensor(offs, dtype=torch.int32, device=rows.device)
        sc, tv, ti = vops.video_scores(rows, off, scores=kind, top_k=self.top_k)
        return sc, tv.cpu().tolist(), ti.cpu().tolist()

    def _call_scored(self, tensor, time_card):
        batched = isinstance(time_card, TimeCardList)
        cards = time_card.time_cards if batched else [time_card]
        offs = [0]
        for tc in cards:
            offs.append(offs[-1] + (self._card_rows(tc) if batched else int(tensor.shape[0])))
        rows = tensor.detach().float()
        k = self.top_k
        empty = ((-1,) * k, (0.0,) * k)
        done_cards, outs = [], []
        if self.aggregate == 1:
            _, tv, ti = self._top(rows, offs, self.scores)
            for v, tc in enumerate(cards):
                out = (tuple(ti[v]), tuple(tv[v]))
                self._emit(tc, *out)
                done_cards.append(tc)
                outs.append(out)
        else:
            # segments add their "_sum" scores (kept on the tensor's device)
            # and row counts per id; the finished totals are ranked together
            sums = self._top(rows, offs, self.scores.replace("mean", "sum"))[0]
            totals, slots, firsts = [], [], []
            for v, tc in enumerate(cards):
                n = offs[v + 1] - offs[v]
                prev = self.results.get(tc.id)
                total = sums[v].clone() if prev is None else prev[0] + sums[v]
                got = [tc] if prev is None else prev[1] + [tc]
                n += 0 if prev is None else prev[2]
                if len(got) < self.aggregate:
                    self.results[tc.id] = (total, got, n)
                    continue
                del self.results[tc.id]
                done_cards.append(TimeCard.merge(got))
                firsts.append(got[0])       # merge() drops extra: the label is read here
                outs.append(empty)
                if n > 0:
                    totals.append(total / n if self.scores.endswith("mean") else total)
                    slots.append(len(outs) - 1)
            if totals:
                _, tv, ti = self._top(torch.stack(totals), list(range(len(totals) + 1)),
                                      "logit_sum")
                for j, slot in enumerate(slots):
                    outs[slot] = (tuple(ti[j]), tuple(tv[j]))
            for tc, out in zip(firsts, outs):
                self._emit(tc, *out)
        if not done_cards:
            return None, None, None
        if not batched:
            return None, outs[0], done_cards[0]
        return None, outs, TimeCardList(done_cards)

    def __call__(self, tensors, non_tensors, time_card):
        tensor = tensors[0]
        if self._scored:
            return self._call_scored(tensor, time_card)
        if isinstance(time_card, TimeCardList):
            cards = time_card.time_cards
            arr = tensor.detach().float().cpu().numpy()
            parts, row = [], 0
            for tc in cards:
                n = tc.extra.get("rows")
                if n is None:
                    n = tc.num_clips if tc.num_clips is not None else 1
                parts.append(arr[row:row + n])
                row += n
        else:
            cards = [time_card]
            parts = [tensor.detach().float().cpu().numpy()]
        done_cards, outs = [], []
        for tc, part in zip(cards, parts):
            result = part.sum(axis=0) if part.shape[0] else \
                np.zeros(tensor.shape[1:], dtype=np.float32)
            if self.aggregate == 1:
                done_cards.append(tc)
                batched = isinstance(time_card, TimeCardList)
                outs.append(int(result.argmax()) if part.shape[0] or not batched else -1)
                if self._tracks(tc):
                    self._emit(tc, (outs[-1],), (float(result[outs[-1]]),))
                continue
            prev = self.results.get(tc.id)
            total = result if prev is None else prev[0] + result
            got = [tc] if prev is None else prev[1] + [tc]
            if len(got) < self.aggregate:
                self.results[tc.id] = (total, got)
                continue
            del self.results[tc.id]
            src = got[0].extra.get("clip_src")
            if src is not None and self._check_dir and self._checked < CHECK_MAX:
                from ...numerics import write_sample
                self._checked += 1
                write_sample(self._check_dir, tc.id, "aggregate", src[0], src[1], total,
                             segments=self.aggregate, clip_length=self.clip_length,
                             step=got[0].extra.get("clip_step", (1, 1)))
            done_cards.append(TimeCard.merge(got))
            outs.append(int(total.argmax()))
            if self._tracks(got[0]):
                self._emit(got[0], (outs[-1],), (float(total[outs[-1]]),))
        if not done_cards:
            return None, None, None
        if not isinstance(time_card, TimeCardList):
            return None, outs[0], done_cards[0]
        return None, outs, TimeCardList(done_cards)

    def input_shape(self):
        return ((DEFAULT_MAX_CLIPS, 400),)

    @staticmethod
    def output_shape():
        return None


class LargeSmallSelector(QueueSelector):
    """Routes 15-clip videos to queue 1 and everything else to queue 0
    (reference config/rnb.json, models/r2p1d/model.py:288-296).

    ``RNB_LARGE_OVERFLOW=k`` (> 0): a 15-clip video goes to queue 0 instead
    while k or more are already waiting in queue 1 -- the one 15-clip replica
    of a GPU cannot drain a burst of them alone, and the 1-clip replicas'
    buckets take whole 15-clip videos too (work-conserving overflow; the
    runner passes the queues to selectors that accept them)."""

    def __init__(self, num_queues, large_clips: int = 15, queues=None):
        if num_queues != 2:
            raise ValueError("LargeSmallSelector needs exactly 2 out queues")
        super().__init__(num_queues)
        self.large_clips = large_clips
        self.queues = queues
        self.overflow = int(os.environ.get("RNB_LARGE_OVERFLOW", "0") or 0)
        self.overflowed = 0

    def select(self, tensors, non_tensors, time_card):
        n = getattr(time_card, "num_clips", None)
        if n is None or n < self.large_clips:
            return 0
        if self.overflow > 0 and self.queues is not None:
            try:
                backlog = self.queues[1].qsize()
            except (NotImplementedError, AttributeError, OSError):
                backlog = 0
            if backlog >= self.overflow:
                self.overflowed += 1
                return 0
        return 1
