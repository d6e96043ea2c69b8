"""The decode SLI tracker on the device (ops/csrc/decodesli.hip, bound in ``_mislo_agent``): per service
a TPOT histogram, the exact TPOT sum and the 2x2 table of requests by (TTFT breach, TPOT breach), for
the window and for a rolling horizon of windows, with the p50 / p90 / p95 / p99 buckets of both. Native
like the window engine (HIP, no PyTorch), on its own stream. The rules, and the host implementation it
is tested against, are pipeline/decodesli.py's.
"""

from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

from .lanecheckpoint import LaneCheckpoint


class DecodeSliTracker(LaneCheckpoint):
    """``step`` per window with the span ranges the engine gets; ``results`` per step index."""

    def __init__(self, span_cap: int = 16384, group_cap: int = 64, windows: int = 150, n_buffers: int = 3,
                 slo_ms: float = 800.0, tpot_slo_ms: float = 100.0, device: int = 0, lds: bool = True):
        """``lds`` False: no per-workgroup LDS table in the observe kernel (the measurement's other side)."""
        from ..pipeline import decodesli as rules
        from . import load_agent

        rules.check_config(int(span_cap), int(group_cap), int(windows), int(n_buffers), float(slo_ms), float(tpot_slo_ms))
        mod = load_agent()
        if not hasattr(mod, "DecodeSliTracker"):
            raise RuntimeError("stale _mislo_agent build: no decode sli (rebuild with ops.build)")
        if (int(mod.DECODESLI_K), int(mod.DECODESLI_STATS), int(mod.DECODESLI_PER_LANE)) != \
                (rules.K, rules.N_STATS, rules.PER_LANE):
            raise RuntimeError("stale _mislo_agent build: decode sli constants differ (rebuild with ops.build)")
        self.span_cap, self.group_cap, self.windows, self.nb = int(span_cap), int(group_cap), int(windows), int(n_buffers)
        self.slo_ms, self.tpot_slo_ms = float(slo_ms), float(tpot_slo_ms)
        self.tpot_slo_us = int(mod.decodesli_tpot_slo_us(float(tpot_slo_ms)))
        self.lds_slots = int(mod.DECODESLI_LDS_SLOTS)
        self.t = mod.DecodeSliTracker(device=int(device), span_cap=int(span_cap), group_cap=int(group_cap),
                                      windows=int(windows), n_buffers=int(n_buffers), slo_ms=float(slo_ms),
                                      tpot_slo_ms=float(tpot_slo_ms), lds=bool(lds))

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
        """Step ``i`` (waits for it): pipeline/decodesli.py RESULT_FIELDS."""
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
        """The rolling state (synchronous): ``rows`` [group_cap, K], ``cells`` [group_cap, 4], ``sum_us``
        [group_cap] and ``pos``, the horizon row the next step replaces."""
        rows, cells, sums, pos = self.t.resident()
        return {"rows": np.asarray(rows, dtype=np.uint32), "cells": np.asarray(cells, dtype=np.uint32),
                "sum_us": np.asarray(sums, dtype=np.uint64), "pos": int(pos)}

    def sync(self) -> None:
        self.t.sync()

    def close(self) -> None:
        self.t.close()
