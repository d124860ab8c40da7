"""Clip sampler for R(2+1)D (reference: models/r2p1d/sampler.py:1-62).

Given a video length, picks ``num_clips`` (weighted choice from
``num_clips_population``; reference default 1 clip w.p. 10/11, 15 clips w.p.
1/11, so E[clips] = 25/11) and returns the start frame of each clip: clips are
spread over the whole video with equal spacing ``floor(len / n)`` and a random
offset in ``[0, leniency]``; if ``clip_length * n`` exceeds the length the
count is reduced until it fits. Same semantics as the reference, without the
NVVL base class (the loader backends consume the start indices directly).

A clip need not be consecutive frames: with a step ``(p, q)`` (a reduced
fraction ``p / q`` of source frames per clip frame) frame ``f`` of a clip is
source frame ``start + (f * p) // q`` -- the nearest lower frame, torchvision's
``floor(i * src_fps / fps)`` resampling. ``clip_frames``, ``clip_span`` and
``step_of`` are the one definition of that; the sampler fits clips by the span
they cover. ``placement="uniform"`` centres the clips instead of drawing the
offset (the deterministic placement of an evaluation run).
"""
from __future__ import annotations

import math
import numbers
import random
from fractions import Fraction
from typing import List, Optional, Sequence, Tuple

PLACEMENTS = ("random", "uniform")


def _check_step(step) -> Tuple[int, int]:
    try:
        p, q = step
    except (TypeError, ValueError):
        raise ValueError("step must be a pair (p, q), got %r" % (step,))
    for v in (p, q):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1:
            raise ValueError("step (p, q) must be positive integers, got %r" % (step,))
    if math.gcd(int(p), int(q)) != 1:
        raise ValueError("step (p, q) must be coprime, got %r" % (step,))
    return int(p), int(q)


def clip_frames(start: int, F: int, step=(1, 1)) -> List[int]:
    """The source frames of an ``F``-frame clip at ``start``: frame ``f`` is
    ``start + (f * p) // q`` for ``step = (p, q)``. ``p / q`` > 1 skips source
    frames, < 1 repeats them."""
    p, q = _check_step(step)
    return [int(start) + (f * p) // q for f in range(F)]


def clip_span(F: int, step=(1, 1)) -> int:
    """Source frames an ``F``-frame clip covers, first to last selected."""
    p, q = _check_step(step)
    return ((F - 1) * p) // q + 1


def parse_rate(rate, what: str = "fps") -> Optional[Fraction]:
    """A frame rate as an exact ``Fraction``: a positive number, an ``"n:d"``
    (or ``"n/d"``) string or an ``(n, d)`` pair; ``None`` stays ``None``. A
    float goes through its shortest decimal string, so 12.5 is 25/2."""
    if rate is None:
        return None
    try:
        if isinstance(rate, bool):
            raise ValueError
        if isinstance(rate, str):
            n, sep, d = rate.replace("/", ":").partition(":")
            val = Fraction(int(n), int(d)) if sep else Fraction(n.strip())
        elif isinstance(rate, (tuple, list)):
            n, d = rate
            if any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in (n, d)):
                raise ValueError
            val = Fraction(int(n), int(d))
        elif isinstance(rate, numbers.Rational):
            val = Fraction(rate)
        elif isinstance(rate, numbers.Real):
            val = Fraction(str(float(rate)))
        else:
            raise ValueError
    except (ValueError, TypeError, ZeroDivisionError):
        raise ValueError("%s = %r is not a frame rate (a positive number or \"n:d\")"
                         % (what, rate))
    if val <= 0:
        raise ValueError("%s = %r must be positive" % (what, rate))
    return val


def check_frame_step(frame_step) -> int:
    if isinstance(frame_step, bool) or not isinstance(frame_step, numbers.Integral) \
            or frame_step < 1:
        raise ValueError("frame_step = %r must be an integer >= 1" % (frame_step,))
    return int(frame_step)


def step_of(frame_step=1, fps=None, source_fps=None) -> Tuple[int, int]:
    """The step ``(p, q)`` of a request: ``(frame_step, 1)``, or with ``fps``
    the exact reduced ``source_fps / fps`` (``source_fps``: an ``(n, d)`` pair),
    never through a float quotient: 30000/1001 to 15 fps is (2000, 1001)."""
    frame_step = check_frame_step(frame_step)
    if fps is None:
        return frame_step, 1
    if frame_step != 1:
        raise ValueError("frame_step = %r and fps = %r: give one of them" % (frame_step, fps))
    target = parse_rate(fps, "fps")
    if source_fps is None:
        raise ValueError("fps = %r needs source_fps, the rate of the file" % (fps,))
    step = parse_rate(source_fps, "source_fps") / target
    return step.numerator, step.denominator


class R2P1DSampler:
    def __init__(self, clip_length: int = 8, num_clips: int = 10,
                 num_clips_population: Optional[Sequence[int]] = (1, 15),
                 num_clips_weights: Optional[Sequence[float]] = (10, 1),
                 seed: Optional[int] = None, placement: str = "random"):
        if placement not in PLACEMENTS:
            raise ValueError("placement = %r, expected one of %s" % (placement, PLACEMENTS))
        self.clip_length = clip_length
        self.num_clips = num_clips
        self.num_clips_population = list(num_clips_population) if num_clips_population else None
        self.num_clips_weights = list(num_clips_weights) if num_clips_weights else None
        self.placement = placement
        self.rng = random.Random(seed)

    def _sample(self, length: int, num_clips: int, span: Optional[int] = None
                ) -> Optional[List[int]]:
        span = self.clip_length if span is None else span
        while num_clips > 0 and span * num_clips > length:
            num_clips -= 1
        if num_clips == 0:
            return None
        stride = int(float(length) / num_clips)
        interval = stride - span
        leniency = interval + (length - stride * num_clips)
        start = leniency // 2 if self.placement == "uniform" else self.rng.randint(0, leniency)
        return [start + i * stride for i in range(num_clips)]

    def choose_num_clips(self) -> int:
        if self.num_clips_population is not None and self.num_clips_weights is not None:
            return self.rng.choices(self.num_clips_population, self.num_clips_weights)[0]
        return self.num_clips

    def sample(self, length: int, span: Optional[int] = None) -> Optional[List[int]]:
        """Clip start frames for a video of ``length`` frames, each clip
        covering ``span`` source frames (default ``clip_length``)."""
        return self._sample(length, self.choose_num_clips(), span)

    def expected_clips(self) -> float:
        if self.num_clips_population is None or self.num_clips_weights is None:
            return float(self.num_clips)
        tot = float(sum(self.num_clips_weights))
        return sum(p * w for p, w in zip(self.num_clips_population,
                                         self.num_clips_weights)) / tot
