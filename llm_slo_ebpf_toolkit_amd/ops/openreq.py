"""The open-request tracker on the device (ops/csrc/openreq.hip, bound in ``_mislo_agent``): a hash
table of the requests that started and have not reported a first token, swept at every window cut
for TTFT deadlines that passed. Native like the window engine (HIP, no PyTorch), on its own
stream. The rules, and the host implementation it is tested against, are pipeline/openreq.py's.
"""

from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

from .lanecheckpoint import LaneCheckpoint


class OpenRequestTable(LaneCheckpoint):
    """``step`` per window with the span ranges the engine gets; ``results`` per step index."""

    def __init__(self, cap: int = 1 << 20, span_cap: int = 16384, group_cap: int = 64, n_buffers: int = 3,
                 slo_ms: float = 800.0, ttl_ms: float = 120000.0, reorder_ms: float = 2000.0, device: int = 0):
        from . import load_agent

        mod = load_agent()
        if not hasattr(mod, "OpenRequests"):
            raise RuntimeError("stale _mislo_agent build: no open-request tracker (rebuild with ops.build)")
        self.cap, self.span_cap, self.group_cap, self.nb = int(cap), int(span_cap), int(group_cap), int(n_buffers)
        self.lds_groups = int(mod.OPENREQ_LDS_GROUPS)
        self.t = mod.OpenRequests(device=int(device), cap=int(cap), span_cap=int(span_cap), group_cap=int(group_cap),
                                  n_buffers=int(n_buffers), slo_ms=float(slo_ms), ttl_ms=float(ttl_ms),
                                  reorder_ms=float(reorder_ms))

    def step(self, span_ranges: Sequence[Tuple[int, int]], cut_ns: int, prev_cut_ns: int, n_groups: int) -> int:
        """One window: ``span_ranges`` = [(host address, bytes)] of 64-byte SPAN records. They are
        copied to the device before this returns; the kernels run behind it. Returns the step's index."""
        return int(self.t.step([(int(a), int(n)) for a, n in span_ranges], int(cut_ns), int(prev_cut_ns),
                               int(n_groups)))

    def step_records(self, spans: np.ndarray, cut_ns: int, prev_cut_ns: int, n_groups: int) -> int:
        spans = np.ascontiguousarray(spans)
        return self.step([(spans.ctypes.data, spans.nbytes)] if len(spans) else [], cut_ns, prev_cut_ns, n_groups)

    def query(self, i: int) -> bool:
        return bool(self.t.query(int(i)))

    def results(self, i: int, n_groups: int) -> Dict[str, np.ndarray]:
        """{"dl": [G, 2], "dup": [G, 3], "stats": [16]} of step ``i`` (waits for it)."""
        return dict(self.t.results(int(i), int(n_groups)))

    def step_ms(self, i: int) -> Tuple[float, float]:
        """Device time of step ``i``: (copy + kernels, kernels alone), ms."""
        a, b = self.t.step_ms(int(i))
        return float(a), float(b)

    def entries(self):
        """The live rows (trace_h, t, grp, state), sorted by trace hash (synchronous)."""
        return tuple(np.asarray(x) for x in self.t.entries())

    def sync(self) -> None:
        self.t.sync()

    def close(self) -> None:
        self.t.close()
