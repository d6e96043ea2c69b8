"""The TTFT sketch on the device (ops/csrc/slisketch.hip, bound in ``_mislo_agent``): per-service
TTFT histograms of the window and of a rolling horizon of windows, their quantile buckets, exact
``le`` counts and sums. Native like the window engine (HIP, no PyTorch), on its own stream. The
rules, and the host implementation it is tested against, are pipeline/slisketch.py's.
"""

from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

from .lanecheckpoint import LaneCheckpoint


class SliSketch(LaneCheckpoint):
    """``step`` per window with the span ranges the engine gets; ``results`` per step index."""

    def __init__(self, span_cap: int = 16384, group_cap: int = 64, windows: int = 150, n_buffers: int = 3,
                 device: int = 0):
        from ..pipeline import slisketch as rules
        from . import load_agent

        mod = load_agent()
        if not hasattr(mod, "SliSketch"):
            raise RuntimeError("stale _mislo_agent build: no TTFT sketch (rebuild with ops.build)")
        if (int(mod.SLISKETCH_K), tuple(mod.SLISKETCH_EDGES), tuple(mod.SLISKETCH_PERMILLE)) != \
                (rules.K, rules.EDGES, rules.PERMILLE):
            raise RuntimeError("stale _mislo_agent build: TTFT sketch constants differ (rebuild with ops.build)")
        self.span_cap, self.group_cap = int(span_cap), int(group_cap)
        self.windows, self.nb = int(windows), int(n_buffers)
        self.t = mod.SliSketch(device=int(device), span_cap=int(span_cap), group_cap=int(group_cap),
                               windows=int(windows), n_buffers=int(n_buffers))

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
        """Step ``i`` (waits for it): pipeline/slisketch.py RESULT_FIELDS."""
        return dict(self.t.results(int(i), int(n_groups)))

    def step_ms(self, i: int) -> Tuple[float, float]:
        """Device time of step ``i``: (copy + kernels, kernels alone), ms."""
        a, b = self.t.step_ms(int(i))
        return float(a), float(b)

    def rolling(self) -> np.ndarray:
        """The rolling histogram [group_cap, K] (synchronous)."""
        return np.asarray(self.t.rolling())

    def window_hist(self) -> np.ndarray:
        """The last step's window histogram [group_cap, K] (synchronous)."""
        return np.asarray(self.t.window_hist())

    def sync(self) -> None:
        self.t.sync()

    def close(self) -> None:
        self.t.close()
