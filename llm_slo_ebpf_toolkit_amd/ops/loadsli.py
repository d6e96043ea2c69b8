"""The load SLI tracker on the device (ops/csrc/loadsli.hip, bound in ``_mislo_agent``): per service a
ring of absolute time bins of request starts, ends and idle time, a prefix scan over it recomputed
every step, and arrivals, completions, busy time, the peak and the surge / slowdown / drop state as
80-byte rows. Native like the window engine (HIP, no PyTorch), on its own stream. The rules, and the
host implementation it is tested against, are pipeline/loadsli.py's.
"""

from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from .lanecheckpoint import LaneCheckpoint


class LoadSliTracker(LaneCheckpoint):
    """``step`` per window with the span ranges the engine gets and the cut's time; ``results`` per
    step index."""

    def __init__(self, bins: int = 1024, bin_us: int = 500_000, settle_bins: int = 30, recent_bins: int = 30,
                 min_base_bins: int = 60, factor_milli: int = 1500, min_requests: int = 20, min_conc_milli: int = 1000,
                 span_cap: int = 16384, group_cap: int = 64, n_buffers: int = 3, ring_records_max: Optional[int] = None,
                 device: int = 0, lds: bool = True):
        """``lds`` False: no per-workgroup LDS table in the observe kernel (the measurement's other side)."""
        from ..pipeline import loadsli as rules
        from . import load_agent

        if ring_records_max is None:
            ring_records_max = rules.default_ring_records_max(max(int(bins), 1), max(int(bin_us), 1))
        rules.check_config(int(bins), int(bin_us), int(settle_bins), int(recent_bins), int(min_base_bins),
                           int(factor_milli), int(min_requests), int(min_conc_milli), int(span_cap), int(group_cap),
                           int(n_buffers), int(ring_records_max))
        mod = load_agent()
        if not hasattr(mod, "LoadSliTracker"):
            raise RuntimeError("stale _mislo_agent build: no load sli (rebuild with ops.build)")
        if (int(mod.LOADSLI_ROW_BYTES), int(mod.LOADSLI_STATS), tuple(mod.LOADSLI_BINS)) != \
                (rules.ROW_BYTES, rules.N_STATS, (rules.MIN_BINS, rules.MAX_BINS)):
            raise RuntimeError("stale _mislo_agent build: load sli constants differ (rebuild with ops.build)")
        self.row = rules.LOAD_ROW
        self.bins, self.bin_us = int(bins), int(bin_us)
        self.settle, self.recent, self.min_base_bins = int(settle_bins), int(recent_bins), int(min_base_bins)
        self.span_cap, self.group_cap, self.nb = int(span_cap), int(group_cap), int(n_buffers)
        self.ring_records_max = int(ring_records_max)
        self.lds_slots = int(mod.LOADSLI_LDS_SLOTS)
        self.t = mod.LoadSliTracker(device=int(device), bins=int(bins), bin_us=int(bin_us), settle_bins=int(settle_bins),
                                    recent_bins=int(recent_bins), min_base_bins=int(min_base_bins),
                                    factor_milli=int(factor_milli), min_requests=int(min_requests),
                                    min_conc_milli=int(min_conc_milli), span_cap=int(span_cap), group_cap=int(group_cap),
                                    n_buffers=int(n_buffers), ring_records_max=int(ring_records_max), lds=bool(lds))

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
        """Step ``i`` (waits for it): pipeline/loadsli.py RESULT_FIELDS."""
        d = dict(self.t.results(int(i), int(n_groups)))
        raw = np.ascontiguousarray(d["rows"])
        d["rows"] = raw.view(self.row).reshape(raw.shape[:-1])
        return d

    def block(self, i: int) -> np.ndarray:
        """Step ``i``'s whole result block (waits for it), uint32 words (pipeline/loadsli.py layout)."""
        return np.asarray(self.t.block(int(i)), dtype=np.uint32)

    def step_ms(self, i: int) -> Tuple[float, float]:
        """Device time of step ``i``: (copy + kernels, kernels alone), ms."""
        a, b, _ = self.t.step_ms(int(i))
        return float(a), float(b)

    def observe_ms(self, i: int) -> float:
        """Device time of step ``i``'s observe kernel alone, ms."""
        return float(self.t.step_ms(int(i))[2])

    def resident(self) -> Dict[str, np.ndarray]:
        """Everything kept between steps (synchronous): ``counts`` / ``idle_us`` [group_cap, B] in slot
        order, ``carry``, ``age``, ``prev_state``, ``q_hi``, ``q_first``."""
        counts, idle, carry, age, prev, q_hi, q_first = self.t.resident()
        return {"counts": np.asarray(counts, dtype=np.uint64), "idle_us": np.asarray(idle, dtype=np.uint64),
                "carry": np.asarray(carry, dtype=np.int32), "age": np.asarray(age, dtype=np.uint32),
                "prev_state": np.asarray(prev, dtype=np.uint32), "q_hi": int(q_hi), "q_first": int(q_first)}

    def sync(self) -> None:
        self.t.sync()

    def close(self) -> None:
        self.t.close()
