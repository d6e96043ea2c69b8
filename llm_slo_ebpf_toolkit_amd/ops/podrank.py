"""The per-pod breach breakdown on the device (ops/csrc/podrank.hip, bound in ``_mislo_agent``): per
service the pods seen, the pods breaching and the pods with the most TTFT breaches of the window and
of the last windows, as 32-byte rows. Native like the window engine (HIP, no PyTorch), on its own
stream. The rules, and the host implementation it is tested against, are pipeline/podrank.py's.
"""

from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

from .lanecheckpoint import LaneCheckpoint


class PodRankTracker(LaneCheckpoint):
    """``step`` per window with the span ranges the engine gets; ``results`` per step index."""

    def __init__(self, k: int = 3, windows: int = 3, pair_cap: int = 4096, span_cap: int = 16384, group_cap: int = 64,
                 n_buffers: int = 3, slo_ms: float = 800.0, device: int = 0, lds: bool = True):
        """``lds`` False: no per-workgroup LDS table in the observe kernel (the measurement's other side)."""
        from ..pipeline import podrank as rules
        from . import load_agent

        rules.check_config(int(k), int(windows), int(pair_cap), int(span_cap), int(group_cap), int(n_buffers),
                           float(slo_ms))
        mod = load_agent()
        if not hasattr(mod, "PodRankTracker"):
            raise RuntimeError("stale _mislo_agent build: no pod breakdown (rebuild with ops.build)")
        if (int(mod.PODRANK_MAX_K), int(mod.PODRANK_MAX_H), int(mod.PODRANK_ROW_BYTES), int(mod.PODRANK_STATS)) != \
                (rules.MAX_K, rules.MAX_H, rules.ROW_BYTES, rules.N_STATS):
            raise RuntimeError("stale _mislo_agent build: pod breakdown constants differ (rebuild with ops.build)")
        self.row, self.pair = rules.POD_ROW, rules.PAIR
        self.k, self.windows, self.pair_cap = int(k), int(windows), int(pair_cap)
        self.span_cap, self.group_cap, self.nb, self.slo_ms = int(span_cap), int(group_cap), int(n_buffers), float(slo_ms)
        self.lds_slots = int(mod.PODRANK_LDS_SLOTS)
        self.t = mod.PodRankTracker(device=int(device), k=int(k), windows=int(windows), pair_cap=int(pair_cap),
                                    span_cap=int(span_cap), group_cap=int(group_cap), n_buffers=int(n_buffers),
                                    slo_ms=float(slo_ms), lds=bool(lds))

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
        """Step ``i`` (waits for it): pipeline/podrank.py RESULT_FIELDS."""
        d = dict(self.t.results(int(i), int(n_groups)))
        for s in ("win_top", "rec_top"):
            raw = np.ascontiguousarray(d[s])
            d[s] = raw.view(self.row).reshape(raw.shape[:-1])
        return d

    def step_ms(self, i: int) -> Tuple[float, float]:
        """Device time of step ``i``: (copy + kernels, kernels alone), ms."""
        a, b, _ = self.t.step_ms(int(i))
        return float(a), float(b)

    def observe_ms(self, i: int) -> float:
        """Device time of step ``i``'s observe kernel alone, ms."""
        return float(self.t.step_ms(int(i))[2])

    def resident(self) -> List[np.ndarray]:
        """The horizon (synchronous): per slot (step % windows) its PAIR list, in no particular order."""
        out = []
        for key, n, b, mx, sm in self.t.resident():
            key = np.asarray(key, dtype=np.uint64)
            p = np.zeros(len(key), self.pair)
            p["g"] = ((key >> np.uint64(32)) - np.uint64(1)).astype(np.uint32) if len(key) else 0
            p["pod"] = (key & np.uint64(0xFFFFFFFF)).astype(np.uint32)
            p["n"], p["b"], p["max_bits"], p["sum_milli"] = n, b, mx, sm
            out.append(p)
        return out

    def sync(self) -> None:
        self.t.sync()

    def close(self) -> None:
        self.t.close()
