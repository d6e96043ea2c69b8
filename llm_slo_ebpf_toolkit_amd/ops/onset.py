"""The breach-onset tracker on the device (ops/csrc/onset.hip, bound in ``_mislo_agent``): per service
a ring of absolute time bins of requests and breaches, an integer CUSUM over it recomputed every step,
and the onset, alarm bin and excess of the current excursion as 64-byte rows. Native like the window
engine (HIP, no PyTorch), on its own stream. The rules, and the host implementation it is tested
against, are pipeline/onset.py's.
"""

from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

from .lanecheckpoint import LaneCheckpoint


class OnsetTracker(LaneCheckpoint):
    """``step`` per window with the span ranges the engine gets and the cut's time; ``results`` per
    step index."""

    def __init__(self, bins: int = 1024, bin_ns: int = 125_000_000, ref_ppm: int = 20000, alarm: int = 3,
                 span_cap: int = 16384, group_cap: int = 64, n_buffers: int = 3, slo_ms: float = 800.0,
                 ring_records_max: int = (1 << 31) - 1, device: int = 0, lds: bool = True):
        """``lds`` False: no per-workgroup LDS table in the observe kernel (the measurement's other side)."""
        from ..pipeline import onset as rules
        from . import load_agent

        rules.check_config(int(bins), int(bin_ns), int(ref_ppm), int(alarm), int(span_cap), int(group_cap),
                           int(n_buffers), float(slo_ms), int(ring_records_max))
        mod = load_agent()
        if not hasattr(mod, "OnsetTracker"):
            raise RuntimeError("stale _mislo_agent build: no breach onset (rebuild with ops.build)")
        if (int(mod.ONSET_ROW_BYTES), int(mod.ONSET_STATS), tuple(mod.ONSET_BINS)) != \
                (rules.ROW_BYTES, rules.N_STATS, (rules.MIN_BINS, rules.MAX_BINS)):
            raise RuntimeError("stale _mislo_agent build: breach onset constants differ (rebuild with ops.build)")
        self.row = rules.ONSET_ROW
        self.bins, self.bin_ns, self.ref_ppm, self.alarm = int(bins), int(bin_ns), int(ref_ppm), int(alarm)
        self.span_cap, self.group_cap, self.nb, self.slo_ms = int(span_cap), int(group_cap), int(n_buffers), float(slo_ms)
        self.lds_slots = int(mod.ONSET_LDS_SLOTS)
        self.t = mod.OnsetTracker(device=int(device), bins=int(bins), bin_ns=int(bin_ns), ref_ppm=int(ref_ppm),
                                  alarm=int(alarm), span_cap=int(span_cap), group_cap=int(group_cap),
                                  n_buffers=int(n_buffers), slo_ms=float(slo_ms),
                                  ring_records_max=int(ring_records_max), lds=bool(lds))

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
        """Step ``i`` (waits for it): pipeline/onset.py RESULT_FIELDS."""
        d = dict(self.t.results(int(i), int(n_groups)))
        raw = np.ascontiguousarray(d["rows"])
        d["rows"] = raw.view(self.row).reshape(raw.shape[:-1])
        return d

    def step_ms(self, i: int) -> Tuple[float, float]:
        """Device time of step ``i``: (copy + kernels, kernels alone), ms."""
        a, b, _ = self.t.step_ms(int(i))
        return float(a), float(b)

    def observe_ms(self, i: int) -> float:
        """Device time of step ``i``'s observe kernel alone, ms."""
        return float(self.t.step_ms(int(i))[2])

    def resident(self) -> Dict[str, np.ndarray]:
        """The whole ring (synchronous): ``n`` / ``b`` [group_cap, B] in slot order, and ``q_hi``."""
        cells, q_hi = self.t.resident()
        cells = np.asarray(cells, dtype=np.uint64)
        return {"n": (cells & np.uint64(0xFFFFFFFF)).astype(np.uint32), "b": (cells >> np.uint64(32)).astype(np.uint32),
                "q_hi": int(q_hi)}

    def sync(self) -> None:
        self.t.sync()

    def close(self) -> None:
        self.t.close()
