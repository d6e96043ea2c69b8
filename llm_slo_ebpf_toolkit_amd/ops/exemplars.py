"""The request-exemplar tracker on the device (ops/csrc/exemplars.hip, bound in ``_mislo_agent``): per
service the records with the largest TTFT of the window and of the last windows, as 64-byte rows.
Native like the window engine (HIP, no PyTorch), on its own stream. The rules, and the host
implementation it is tested against, are pipeline/exemplars.py's.
"""

from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

from .lanecheckpoint import LaneCheckpoint


class ExemplarTracker(LaneCheckpoint):
    """``step`` per window with the span ranges the engine gets; ``results`` per step index."""

    def __init__(self, k: int = 3, windows: int = 3, span_cap: int = 16384, group_cap: int = 64, n_buffers: int = 3,
                 device: int = 0, lds: bool = True):
        """``lds`` False: no LDS privatisation in the select kernel (the measurement's other side)."""
        from ..pipeline import exemplars as rules
        from . import load_agent

        rules.check_config(int(k), int(windows), int(span_cap), int(group_cap), int(n_buffers))
        mod = load_agent()
        if not hasattr(mod, "ExemplarTracker"):
            raise RuntimeError("stale _mislo_agent build: no request exemplars (rebuild with ops.build)")
        if (int(mod.EXEMPLAR_MAX_K), int(mod.EXEMPLAR_MAX_H), int(mod.EXEMPLAR_ROW_BYTES), int(mod.EXEMPLAR_STATS)) != \
                (rules.MAX_K, rules.MAX_H, rules.ROW_BYTES, rules.N_STATS):
            raise RuntimeError("stale _mislo_agent build: request exemplar constants differ (rebuild with ops.build)")
        self.row = rules.EXEMPLAR
        self.k, self.windows, self.span_cap, self.group_cap = int(k), int(windows), int(span_cap), int(group_cap)
        self.nb = int(n_buffers)
        self.lds_groups = int(mod.EXEMPLAR_LDS_GROUPS)
        self.t = mod.ExemplarTracker(device=int(device), k=int(k), windows=int(windows), span_cap=int(span_cap),
                                     group_cap=int(group_cap), n_buffers=int(n_buffers), lds=bool(lds))

    def step(self, span_ranges: Sequence[Tuple[int, int]], n_groups: int) -> int:
        """One window: ``span_ranges`` = [(host address, bytes)] of 64-byte SPAN records. They are
        copied to the device before this returns; the kernels run behind it. Returns the step's index."""
        return int(self.t.step([(int(a), int(n)) for a, n in span_ranges], int(n_groups)))

    def step_records(self, spans: np.ndarray, n_groups: int) -> int:
        spans = np.ascontiguousarray(spans)
        return self.step([(spans.ctypes.data, spans.nbytes)] if len(spans) else [], n_groups)

    def query(self, i: int) -> bool:
        return bool(self.t.query(int(i)))

    def _rows(self, raw) -> np.ndarray:
        raw = np.ascontiguousarray(raw)
        return raw.view(self.row).reshape(raw.shape[:-1])

    def results(self, i: int, n_groups: int) -> Dict[str, np.ndarray]:
        """Step ``i`` (waits for it): pipeline/exemplars.py RESULT_FIELDS."""
        d = dict(self.t.results(int(i), int(n_groups)))
        d["win"], d["recent"] = self._rows(d["win"]), self._rows(d["recent"])
        return d

    def step_ms(self, i: int) -> Tuple[float, float]:
        """Device time of step ``i``: (copy + kernels, kernels alone), ms."""
        a, b, _ = self.t.step_ms(int(i))
        return float(a), float(b)

    def select_ms(self, i: int) -> float:
        """Device time of step ``i``'s select kernel alone, ms."""
        return float(self.t.step_ms(int(i))[2])

    def resident(self) -> Dict[str, np.ndarray]:
        """The horizon (synchronous): ``rows`` [windows, group_cap, k], ``k`` [windows, group_cap]."""
        rows, held = self.t.resident()
        return {"rows": self._rows(rows), "k": np.asarray(held)}

    def sync(self) -> None:
        self.t.sync()

    def close(self) -> None:
        self.t.close()
