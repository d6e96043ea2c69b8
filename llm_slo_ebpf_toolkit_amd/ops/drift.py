"""The TTFT drift tracker on the device (ops/csrc/drift.hip, bound in ``_mislo_agent``): per service a
recent TTFT histogram, a trailing baseline of calm windows and, every window, an integer one-sided
two-sample Kolmogorov-Smirnov decision on whether the recent distribution is slower or faster. Native
like the window engine (HIP, no PyTorch), on its own stream. The rules, and the host implementation it
is tested against, are pipeline/drift.py's.
"""

from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from .lanecheckpoint import LaneCheckpoint


class DriftTracker(LaneCheckpoint):
    """``step`` per window with the span ranges the engine gets; ``results`` per step index."""

    def __init__(self, span_cap: int = 16384, group_cap: int = 64, recent: int = 10, gap: int = 10, baseline: int = 300,
                 n_buffers: int = 3, crit: Optional[float] = None, min_shift: Optional[int] = None,
                 min_recent: Optional[int] = None, min_base: Optional[int] = None,
                 min_base_windows: Optional[int] = None, hold_max: Optional[int] = None, device: int = 0,
                 lds: bool = True):
        """``lds`` False: no per-workgroup LDS table in the observe kernel (the measurement's other side)."""
        from ..pipeline import drift as rules
        from . import load_agent

        self.cfg = rules.resolve(recent, gap, baseline, crit, min_shift, min_recent, min_base, min_base_windows, hold_max)
        rules.check_config(int(span_cap), int(group_cap), n_buffers=int(n_buffers), **self.cfg)
        mod = load_agent()
        if not hasattr(mod, "DriftTracker"):
            raise RuntimeError("stale _mislo_agent build: no ttft drift (rebuild with ops.build)")
        if (int(mod.DRIFT_K), int(mod.DRIFT_ROW_STRIDE), int(mod.DRIFT_STATS), int(mod.DRIFT_PER_LANE)) != \
                (rules.K, rules.ROW_STRIDE, rules.N_STATS, rules.PER_LANE):
            raise RuntimeError("stale _mislo_agent build: ttft drift constants differ (rebuild with ops.build)")
        self.span_cap, self.group_cap, self.nb = int(span_cap), int(group_cap), int(n_buffers)
        self.R, self.L, self.B = self.cfg["recent"], self.cfg["gap"], self.cfg["baseline"]
        self.crit_q = int(mod.drift_crit_q(self.cfg["crit"]))
        self.lds_slots = int(mod.DRIFT_LDS_SLOTS)
        self.t = mod.DriftTracker(device=int(device), span_cap=int(span_cap), group_cap=int(group_cap),
                                  n_buffers=int(n_buffers), lds=bool(lds), **self.cfg)

    def step(self, span_ranges: Sequence[Tuple[int, int]], n_groups: int) -> int:
        """One window: ``span_ranges`` = [(host address, bytes)] of 64-byte SPAN records. They are
        copied to the device before this returns; the kernels run behind it. Returns the step's index."""
        return int(self.t.step([(int(a), int(n)) for a, n in span_ranges], int(n_groups)))

    def step_records(self, spans: np.ndarray, n_groups: int) -> int:
        spans = np.ascontiguousarray(spans)
        return self.step([(spans.ctypes.data, spans.nbytes)] if len(spans) else [], n_groups)

    def query(self, i: int) -> bool:
        return bool(self.t.query(int(i)))

    def results(self, i: int, n_groups: int) -> Dict[str, np.ndarray]:
        """Step ``i`` (waits for it): pipeline/drift.py RESULT_FIELDS."""
        return dict(self.t.results(int(i), int(n_groups)))

    def block(self, i: int) -> np.ndarray:
        """Step ``i``'s whole result block as it left the device (uint32 words; waits for it)."""
        return np.asarray(self.t.block(int(i)), dtype=np.uint32)

    def step_ms(self, i: int) -> Tuple[float, float]:
        """Device time of step ``i``: (copy + kernels, kernels alone), ms."""
        a, b, _ = self.t.step_ms(int(i))
        return float(a), float(b)

    def observe_ms(self, i: int) -> float:
        """Device time of step ``i``'s observe kernel alone, ms (0 for an empty step: not launched)."""
        return float(self.t.step_ms(int(i))[2])

    def resident(self) -> Dict[str, np.ndarray]:
        """The rolling state (synchronous): ``recent`` / ``base`` [group_cap, ROW_STRIDE], ``base_fill`` /
        ``base_pos`` / ``hold`` [group_cap] and ``pos``, the near-ring row the next step replaces."""
        recent, base, fill, pos_b, hold, pos = self.t.resident()
        u = lambda a: np.asarray(a, dtype=np.uint32)  # noqa: E731
        return {"recent": u(recent), "base": u(base), "base_fill": u(fill), "base_pos": u(pos_b), "hold": u(hold),
                "pos": int(pos)}

    def sync(self) -> None:
        self.t.sync()

    def close(self) -> None:
        self.t.close()
