"""The TTFT phase split tracker on the device (ops/csrc/retrsli.hip, bound in ``_mislo_agent``): per service
a histogram of the retrieval time and one of the model time (TTFT minus retrieval), their exact sums, six
counters of requests by TTFT-breach phase and the SLI records seen, for the window and for a rolling horizon
of windows, with the p50 / p90 / p95 / p99 buckets of both histograms and a verdict over the horizon. Native
like the window engine (HIP, no PyTorch), on its own stream. The rules, and the host implementation it is
tested against, are pipeline/retrsli.py's.
"""

from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

from .lanecheckpoint import LaneCheckpoint


class RetrievalSliTracker(LaneCheckpoint):
    """``step`` per window with the span ranges the engine gets; ``results`` per step index."""

    def __init__(self, span_cap: int = 16384, group_cap: int = 64, windows: int = 150, n_buffers: int = 3,
                 slo_ms: float = 800.0, retrieval_budget_ms: float = 200.0, budget_ppm: int = 10000,
                 coverage_ppm: int = 500000, dominance_ppm: int = 667000, min_requests: int = 200, device: int = 0,
                 lds: bool = True):
        """``lds`` False: no per-workgroup LDS table in the observe kernel (the measurement's other side)."""
        from ..pipeline import retrsli as rules
        from . import load_agent

        rules.check_config(int(span_cap), int(group_cap), int(windows), int(n_buffers), float(slo_ms),
                           float(retrieval_budget_ms), int(budget_ppm), int(coverage_ppm), int(dominance_ppm),
                           int(min_requests))
        mod = load_agent()
        if not hasattr(mod, "RetrievalSliTracker"):
            raise RuntimeError("stale _mislo_agent build: no retrieval sli (rebuild with ops.build)")
        if (int(mod.RETRSLI_K), int(mod.RETRSLI_STATS), int(mod.RETRSLI_CELLS), int(mod.RETRSLI_UNIT_MAX)) != \
                (rules.K, rules.N_STATS, rules.N_CELLS, rules.UNIT_MAX):
            raise RuntimeError("stale _mislo_agent build: retrieval sli constants differ (rebuild with ops.build)")
        self.span_cap, self.group_cap, self.windows, self.nb = int(span_cap), int(group_cap), int(windows), int(n_buffers)
        self.slo_ms, self.retrieval_budget_ms = float(slo_ms), float(retrieval_budget_ms)
        self.slo_units = int(mod.retrsli_units_of_ms(float(np.float32(slo_ms))))
        self.budget_units = int(mod.retrsli_budget_units(float(retrieval_budget_ms)))
        self.lds_slots = int(mod.RETRSLI_LDS_SLOTS)
        self.t = mod.RetrievalSliTracker(device=int(device), span_cap=int(span_cap), group_cap=int(group_cap),
                                         windows=int(windows), n_buffers=int(n_buffers), slo_ms=float(slo_ms),
                                         retrieval_budget_ms=float(retrieval_budget_ms), budget_ppm=int(budget_ppm),
                                         coverage_ppm=int(coverage_ppm), dominance_ppm=int(dominance_ppm),
                                         min_requests=int(min_requests), lds=bool(lds))

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
        """Step ``i`` (waits for it): pipeline/retrsli.py RESULT_FIELDS."""
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
        """The rolling state (synchronous): ``rows_r`` / ``rows_m`` [group_cap, K], ``cells`` [group_cap, 6],
        ``sli`` [group_cap], ``sums`` [group_cap, 2] (retrieval, TTFT), ``state``, ``age`` and ``pos``, the
        horizon row the next step replaces."""
        rows_r, rows_m, cells, sli, sums, state, age, pos = self.t.resident()
        return {"rows_r": np.asarray(rows_r, dtype=np.uint32), "rows_m": np.asarray(rows_m, dtype=np.uint32),
                "cells": np.asarray(cells, dtype=np.uint32), "sli": np.asarray(sli, dtype=np.uint32),
                "sums": np.asarray(sums, dtype=np.uint64), "state": np.asarray(state, dtype=np.uint32),
                "age": np.asarray(age, dtype=np.uint32), "pos": int(pos)}

    def sync(self) -> None:
        self.t.sync()

    def close(self) -> None:
        self.t.close()
