"""The error SLI tracker on the device (ops/csrc/errsli.hip, bound in ``_mislo_agent``): per service the
finished requests by outcome class, for the window and for a rolling horizon of windows, and which of
up to four (long window, short window, factor) burn-rate pairs of the availability budget fire. Native
like the window engine (HIP, no PyTorch), on its own stream. The rules, and the host implementation it
is tested against, are pipeline/errsli.py's.
"""

from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

from .lanecheckpoint import LaneCheckpoint


class ErrorSliTracker(LaneCheckpoint):
    """``step`` per window with the span ranges the engine gets; ``results`` per step index."""

    def __init__(self, span_cap: int = 16384, group_cap: int = 64, windows: int = 3600, n_buffers: int = 3,
                 target: float = 0.999, pairs: Sequence[Tuple[int, int, int]] = ((3600, 300, 14400),),
                 min_requests: int = 20, bad_mask: int = 0xF8, device: int = 0, lds: bool = True):
        """``lds`` False: no per-workgroup LDS table in the observe kernel (the measurement's other side)."""
        from ..pipeline import errsli as rules
        from . import load_agent

        pairs = rules._pairs(pairs)
        rules.check_config(int(span_cap), int(group_cap), int(windows), int(n_buffers), float(target), pairs,
                           int(min_requests), int(bad_mask))
        mod = load_agent()
        if not hasattr(mod, "ErrorSliTracker"):
            raise RuntimeError("stale _mislo_agent build: no error sli (rebuild with ops.build)")
        if (int(mod.ERRSLI_CLASSES), int(mod.ERRSLI_MAX_PAIRS), int(mod.ERRSLI_STATS)) != \
                (rules.N_CLASSES, rules.MAX_PAIRS, rules.N_STATS):
            raise RuntimeError("stale _mislo_agent build: error sli constants differ (rebuild with ops.build)")
        self.span_cap, self.group_cap, self.windows, self.nb = int(span_cap), int(group_cap), int(windows), int(n_buffers)
        self.target, self.pairs, self.min_requests, self.bad_mask = float(target), pairs, int(min_requests), int(bad_mask)
        self.lds_slots = int(mod.ERRSLI_LDS_SLOTS)
        self.t = mod.ErrorSliTracker(device=int(device), span_cap=int(span_cap), group_cap=int(group_cap),
                                     windows=int(windows), n_buffers=int(n_buffers), target=float(target), pairs=pairs,
                                     min_requests=int(min_requests), bad_mask=int(bad_mask), lds=bool(lds))
        self.budget_ppm = int(self.t.budget_ppm())

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
        """Step ``i`` (waits for it): pipeline/errsli.py RESULT_FIELDS."""
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
        """The rolling state (synchronous): ``counts`` [group_cap, 8], ``pair_sums`` [group_cap, 4, 4],
        ``age`` [group_cap] and ``pos``, the horizon row the next step replaces."""
        counts, sums, age, pos = self.t.resident()
        return {"counts": np.asarray(counts, dtype=np.uint32), "pair_sums": np.asarray(sums, dtype=np.uint32),
                "age": np.asarray(age, dtype=np.uint32), "pos": int(pos)}

    def sync(self) -> None:
        self.t.sync()

    def close(self) -> None:
        self.t.close()
