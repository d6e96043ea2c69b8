"""The saturation curve tracker on the device (ops/csrc/satcurve.hip, bound in ``_mislo_agent``): per
service the load tracker's ring of time bins with a third cell of requests and TTFT breaches by the bin
they started in, two generations of evicted bins by concurrency level, and every step the merged curve,
its knee and the recent concurrency against it as 64-byte rows. Native like the window engine (HIP, no
PyTorch), on its own stream. The rules, and the host implementation it is tested against, are
pipeline/satcurve.py's.
"""

from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from .lanecheckpoint import LaneCheckpoint


class SaturationTracker(LaneCheckpoint):
    """``step`` per window with the span ranges the engine gets and the cut's time; ``results`` per
    step index."""

    def __init__(self, bins: int = 1024, bin_us: int = 500_000, settle_bins: int = 30, recent_bins: int = 30,
                 epoch_bins: int = 43200, budget_ppm: int = 10000, min_requests: int = 200, slo_ms: float = 800.0,
                 span_cap: int = 16384, group_cap: int = 64, n_buffers: int = 3, ring_records_max: Optional[int] = None,
                 curve_records_max: Optional[int] = None, device: int = 0, lds: bool = True):
        """``lds`` False: no per-workgroup LDS table in the observe kernel (the measurement's other side)."""
        from ..pipeline import satcurve as rules
        from . import load_agent

        if ring_records_max is None:
            ring_records_max = rules.default_ring_records_max(max(int(bins), 1), max(int(bin_us), 1))
        if curve_records_max is None:
            curve_records_max = rules.MAX_CURVE_RECORDS
        rules.check_config(int(bins), int(bin_us), int(settle_bins), int(recent_bins), int(epoch_bins), int(budget_ppm),
                           int(min_requests), float(slo_ms), int(span_cap), int(group_cap), int(n_buffers),
                           int(ring_records_max), int(curve_records_max))
        mod = load_agent()
        if not hasattr(mod, "SaturationTracker"):
            raise RuntimeError("stale _mislo_agent build: no saturation curve (rebuild with ops.build)")
        if (int(mod.SATCURVE_ROW_BYTES), int(mod.SATCURVE_STATS), int(mod.SATCURVE_LEVELS), tuple(mod.SATCURVE_BINS)) != \
                (rules.ROW_BYTES, rules.N_STATS, rules.K, (rules.MIN_BINS, rules.MAX_BINS)):
            raise RuntimeError("stale _mislo_agent build: saturation curve constants differ (rebuild with ops.build)")
        self.row = rules.SAT_ROW
        self.bins, self.bin_us = int(bins), int(bin_us)
        self.settle, self.recent, self.epoch_bins = int(settle_bins), int(recent_bins), int(epoch_bins)
        self.span_cap, self.group_cap, self.nb = int(span_cap), int(group_cap), int(n_buffers)
        self.ring_records_max, self.curve_records_max = int(ring_records_max), int(curve_records_max)
        self.lds_slots = int(mod.SATCURVE_LDS_SLOTS)
        self.t = mod.SaturationTracker(device=int(device), bins=int(bins), bin_us=int(bin_us), settle_bins=int(settle_bins),
                                       recent_bins=int(recent_bins), epoch_bins=int(epoch_bins),
                                       budget_ppm=int(budget_ppm), min_requests=int(min_requests), slo_ms=float(slo_ms),
                                       span_cap=int(span_cap), group_cap=int(group_cap), n_buffers=int(n_buffers),
                                       ring_records_max=int(ring_records_max),
                                       curve_records_max=int(curve_records_max), lds=bool(lds))

    def step(self, span_ranges: Sequence[Tuple[int, int]], cut_ns: int, n_groups: int) -> int:
        """One window: ``span_ranges`` = [(host address, bytes)] of 64-byte SPAN records, cut at
        ``cut_ns`` (> 0). They are copied to the device before this returns; the kernels run behind
        it. Returns the step's index."""
        return int(self.t.step([(int(a), int(n)) for a, n in span_ranges], int(cut_ns), int(n_groups)))

    def step_records(self, spans: np.ndarray, cut_ns: int, n_groups: int) -> int:
        spans = np.ascontiguousarray(spans)
        return self.step([(spans.ctypes.data, spans.nbytes)] if len(spans) else [], cut_ns, n_groups)

    def query(self, i: int) -> bool:
        return bool(self.t.query(int(i)))

    def results(self, i: int, n_groups: int) -> Dict[str, np.ndarray]:
        """Step ``i`` (waits for it): pipeline/satcurve.py RESULT_FIELDS."""
        d = dict(self.t.results(int(i), int(n_groups)))
        raw = np.ascontiguousarray(d["rows"])
        d["rows"] = raw.view(self.row).reshape(raw.shape[:-1])
        return d

    def block(self, i: int) -> np.ndarray:
        """Step ``i``'s whole result block (waits for it), uint32 words (pipeline/satcurve.py layout)."""
        return np.asarray(self.t.block(int(i)), dtype=np.uint32)

    def step_ms(self, i: int) -> Tuple[float, float]:
        """Device time of step ``i``: (copy + kernels, kernels alone), ms."""
        a, b, _ = self.t.step_ms(int(i))
        return float(a), float(b)

    def observe_ms(self, i: int) -> float:
        """Device time of step ``i``'s observe kernel alone, ms."""
        return float(self.t.step_ms(int(i))[2])

    def resident(self) -> Dict[str, object]:
        """Everything kept between steps (synchronous): ``counts`` / ``idle_us`` / ``sli`` [group_cap, B] in
        slot order, ``carry``, ``gen`` [2, group_cap, K, 2], ``gen_epoch``, ``age``, ``q_hi``, ``q_first``."""
        counts, idle, sli, carry, gen, gen_epoch, age, q_hi, q_first = self.t.resident()
        return {"counts": np.asarray(counts, dtype=np.uint64), "idle_us": np.asarray(idle, dtype=np.uint64),
                "sli": np.asarray(sli, dtype=np.uint64), "carry": np.asarray(carry, dtype=np.int32),
                "gen": np.asarray(gen, dtype=np.uint64), "gen_epoch": tuple(int(x) for x in gen_epoch),
                "age": np.asarray(age, dtype=np.uint32), "q_hi": int(q_hi), "q_first": int(q_first)}

    def sync(self) -> None:
        self.t.sync()

    def close(self) -> None:
        self.t.close()
