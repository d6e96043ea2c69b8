"""Worst-TTFT request exemplars per service on the host: the rules of the exemplar tracker.

The window engines reduce every TTFT to counters and the TTFT sketch to histograms; neither keeps an
identity. Per step (one window, the span ranges the engine gets) the tracker yields, per service
(incident group):

* **window**: the ``K`` records with the largest TTFT of this window,
* **recent**: the ``K`` largest over the last ``H`` steps, this one included (the horizon is counted
  in steps like the sketch's: every step ages every row of ``group_cap``, whether or not the group
  is present).

``ExemplarOracle`` is the rules in numpy: the reference the device tracker (ops/csrc/exemplars.hip,
ops/exemplars.py) is tested against for equality, and what ``engine="cpu"`` uses.

**Which records count**: the sketch's observed set. A 64-byte SPAN without SPAN_NO_SLI, with
``group_id < n_groups`` and ``ttft_ms >= 0`` in a float compare; NaN and negatives are ``invalid``,
groups at or above ``n_groups`` are ``out_of_group``, SPAN_LATE records count by their value.

**Order within a window**: larger TTFT first, equal TTFTs to the earlier record, where a record's
index ``i`` is its position in the step's ranges concatenated in the order given. One 64-bit key says
both: ``key = (ord(v) << 32) | (0xFFFFFFFF - i)`` with ``ord(v) = float bits & 0x7fffffff``. For the
accepted values the bit order is the value order and +inf sorts highest; -0.0 passes ``>= 0`` and
ranks as 0 (the mask). Key 0 means empty; no real key is 0 (``i < 2^31``).

**Order across windows** (recent): larger TTFT first, then the newer window, then the earlier position
in its window's list: ``(ord(v) << 32) | 1 << 16 | (15 - age) << 8 | (7 - position)``.

Keys are unique, so every result is a total order: device and oracle are compared for equality.
"""

from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

from ..collector import records
from .trackerstate import OracleCheckpoint

MAX_K = 8                    # exemplars per service and list
MAX_H = 16                   # windows of the horizon: H * K <= 128, two candidates per lane of one wave
ROW_BYTES = 64
# one exemplar (ops/csrc/exemplars_host.h Row)
EXEMPLAR = np.dtype([
    ("ts_ns", "<i8"), ("trace_h", "<u8"), ("span_h", "<u8"),
    ("ttft_ms", "<f4"), ("latency_ms", "<f4"), ("retr_ms", "<f4"),
    ("pod_id", "<u4"), ("pid", "<u4"), ("flags", "<u4"),
    ("age", "<u4"),          # windows ago; 0 in a window row
    ("index", "<u4"),        # the record's index in its step
    ("pad", "<u4", (2,)),
])
assert EXEMPLAR.itemsize == ROW_BYTES
# per-step statistics, in the device's order (ops/csrc/exemplars_host.h Stat)
STATS = ("observed", "invalid", "out_of_group")
N_STATS = 8
EVENT_STATS = ("invalid", "out_of_group")
RESULT_FIELDS = ("n", "k_win", "k_recent", "win", "recent", "stats")
# what WindowPipeline.results() gains with the tracker on
RESULT_KEYS = ("ex_n", "ex_k_win", "ex_win", "ex_k_recent", "ex_recent")


def stats_dict(stats: np.ndarray) -> Dict[str, int]:
    return {name: int(stats[i]) for i, name in enumerate(STATS)}


def ord_of(v) -> np.ndarray:
    """uint64: the float32's bits without the sign -- the value order of the accepted TTFTs."""
    x = np.ascontiguousarray(np.asarray(v, dtype=np.float32))
    return (x.reshape(-1).view(np.uint32) & np.uint32(0x7FFFFFFF)).astype(np.uint64).reshape(x.shape)


def window_keys(v, index) -> np.ndarray:
    """uint64: ``(ord(v) << 32) | (0xFFFFFFFF - index)``."""
    return (ord_of(v) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(index, dtype=np.uint64))


def result_keys(result: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """A step's results under the names WindowPipeline.results() carries (RESULT_KEYS)."""
    return {"ex_n": np.asarray(result["n"]), "ex_k_win": np.asarray(result["k_win"]),
            "ex_win": np.asarray(result["win"]), "ex_k_recent": np.asarray(result["k_recent"]),
            "ex_recent": np.asarray(result["recent"])}


def empty_result(n_groups: int, k: int) -> Dict[str, np.ndarray]:
    G = int(n_groups)
    return {"n": np.zeros(G, np.uint32), "k_win": np.zeros(G, np.uint32), "k_recent": np.zeros(G, np.uint32),
            "win": np.zeros((G, int(k)), EXEMPLAR), "recent": np.zeros((G, int(k)), EXEMPLAR),
            "stats": np.zeros(N_STATS, np.uint32)}


def check_config(k: int, windows: int, span_cap: int, group_cap: int, n_buffers: int) -> None:
    """The configuration checks of ops/csrc/exemplars_host.h validate()."""
    if not 1 <= k <= MAX_K:
        raise ValueError("request exemplars: k must be in [1, 8]")
    if not 1 <= windows <= MAX_H:
        raise ValueError("request exemplars: windows must be in [1, 16]")
    if not 1 <= group_cap <= 65536:
        raise ValueError("request exemplars: group_cap must be in [1, 65536]")
    if not 1 <= span_cap < 1 << 31:
        raise ValueError("request exemplars: span_cap must be in [1, 2^31)")
    if not 1 <= n_buffers <= 64:
        raise ValueError("request exemplars: n_buffers out of range")
    if (windows + 2) * group_cap * k * ROW_BYTES > 1 << 31:
        raise ValueError("request exemplars: the rows of windows x group_cap x k need more than 2 GiB")


def _gather(ranges) -> np.ndarray:
    from .cpu import _gather as g

    b = g(ranges)
    return b.view(records.SPAN) if len(b) else np.zeros(0, records.SPAN)


def rows_of(spans: np.ndarray, index: np.ndarray) -> np.ndarray:
    """EXEMPLAR rows of the records ``spans[index]`` (age 0)."""
    s = spans[index]
    r = np.zeros(len(index), EXEMPLAR)
    for f in ("ts_ns", "trace_h", "span_h", "ttft_ms", "latency_ms", "retr_ms", "pod_id", "pid", "flags"):
        r[f] = s[f]
    r["index"] = index
    return r


class ExemplarOracle(OracleCheckpoint):
    """The tracker's rules in numpy (see the module docstring), with the device handle's interface."""

    # checkpoint (pipeline/trackerstate.py): the fields ops/csrc/exemplars_host.h fingerprint() covers, and what is
    # kept between steps
    KIND = "request exemplars"
    FINGERPRINT = ("group_cap", "windows", "k")
    STATE = ("rows", "held", "n")

    def __init__(self, k: int = 3, windows: int = 3, span_cap: int = 16384, group_cap: int = 64, n_buffers: int = 3,
                 device: int = 0):
        k, windows, span_cap, group_cap, n_buffers = int(k), int(windows), int(span_cap), int(group_cap), int(n_buffers)
        check_config(k, windows, span_cap, group_cap, n_buffers)
        self.k, self.windows, self.span_cap, self.group_cap, self.nb = k, windows, span_cap, group_cap, n_buffers
        self.rows = np.zeros((windows, group_cap, k), EXEMPLAR)  # the horizon: slot step % windows
        self.held = np.zeros((windows, group_cap), np.uint32)    # valid rows of each slot
        self.res: Dict[int, Tuple[int, dict]] = {}
        self.n = 0

    # ---- one window ---------------------------------------------------------------------------
    def step(self, span_ranges: Sequence[Tuple[int, int]], n_groups: int) -> int:
        """``span_ranges`` = [(host address, bytes)] of 64-byte SPAN records, as the engine gets them."""
        for _a, nbytes in span_ranges:
            if int(nbytes) % 64:
                raise ValueError("request exemplars step: a range is not whole 64-byte spans")
        return self.step_records(_gather(span_ranges), n_groups)

    def step_records(self, spans: np.ndarray, n_groups: int) -> int:
        G, C, K, H = int(n_groups), self.group_cap, self.k, self.windows
        if not 0 <= G <= C:
            raise ValueError("request exemplars step: n_groups out of range")
        if len(spans) > self.span_cap:
            raise ValueError("request exemplars step: more spans than span_cap")
        grp = spans["group_id"].astype(np.int64)
        v = np.ascontiguousarray(spans["ttft_ms"], dtype=np.float32)
        sli = (spans["flags"] & np.uint32(records.SPAN_NO_SLI)) == 0
        counts = sli & (grp < G)
        with np.errstate(invalid="ignore"):
            ok = counts & (v >= np.float32(0.0))
        stats = np.zeros(N_STATS, np.uint32)
        stats[:len(STATS)] = [int(ok.sum()), int((counts & ~ok).sum()), int((sli & (grp >= G)).sum())]
        at = np.nonzero(ok)[0]
        keys = window_keys(v[at], at)
        # the K largest keys of every group, in order
        by_key = np.argsort(keys)[::-1]
        by_group = by_key[np.argsort(grp[at][by_key], kind="stable")]
        g_sorted = grp[at][by_group]
        n = np.bincount(g_sorted, minlength=C).astype(np.uint32)
        first = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
        pos = np.arange(len(g_sorted)) - first[g_sorted]
        keep = pos < K
        win = np.zeros((C, K), EXEMPLAR)
        win[g_sorted[keep], pos[keep]] = rows_of(spans, at[by_group[keep]])
        k_win = np.minimum(n, K).astype(np.uint32)

        idx = self.n
        cur = idx % H
        self.rows[cur], self.held[cur] = win, k_win
        # the horizon's H * K candidates of every group by the cross-window order
        age = ((cur - np.arange(H)) % H).astype(np.uint64)
        p = np.arange(K, dtype=np.uint64)
        valid = p[None, None, :] < self.held[:, :, None]
        ck = (ord_of(self.rows["ttft_ms"]) << np.uint64(32)) | np.uint64(1 << 16) \
            | ((np.uint64(15) - age)[:, None, None] << np.uint64(8)) | (np.uint64(7) - p)[None, None, :]
        ck = np.where(valid, ck, np.uint64(0)).transpose(1, 0, 2).reshape(C, H * K)
        order = np.argsort(ck, axis=1)[:, ::-1][:, :K]
        got = np.take_along_axis(ck, order, axis=1) != 0
        recent = self.rows.transpose(1, 0, 2).reshape(C, H * K)[np.arange(C)[:, None], order]
        recent["age"] = age[order // K].astype(np.uint32)
        recent[~got] = np.zeros((), EXEMPLAR)
        res = {"n": n, "k_win": k_win, "k_recent": got.sum(axis=1).astype(np.uint32), "win": win, "recent": recent,
               "stats": stats}
        self.res[idx % self.nb] = (idx, res)
        self.n += 1
        return idx

    # ---- results ------------------------------------------------------------------------------
    def query(self, i: int) -> bool:
        return True

    def results(self, i: int, n_groups: int) -> Dict[str, np.ndarray]:
        held = self.res.get(int(i) % self.nb)
        if held is None or held[0] != int(i):
            raise IndexError(f"request exemplars step {i} is not held (only the last {self.nb})")
        G = int(n_groups)
        if not 0 <= G <= self.group_cap:
            raise ValueError("n_groups")
        return {k: (v.copy() if k == "stats" else v[:G].copy()) for k, v in held[1].items()}

    def step_ms(self, i: int) -> Tuple[float, float]:
        return 0.0, 0.0

    def resident(self) -> Dict[str, np.ndarray]:
        """The horizon: ``rows`` [windows, group_cap, k] (slot = step % windows, age 0) and ``k``
        [windows, group_cap], the valid rows of each."""
        return {"rows": self.rows.copy(), "k": self.held.copy()}

    def sync(self) -> None:
        pass

    def close(self) -> None:
        pass
