"""Per-service TTFT distributions on the host: the rules of the TTFT sketch.

The window engines reduce every TTFT to ``sli[g] = (requests, breaches)``; the sketch keeps the
value. Per step (one window, the span ranges the engine gets) it yields, per service (incident
group): the window's histogram and the histogram of the last ``windows`` steps (the rolling
horizon), the p50 / p90 / p95 / p99 buckets of both, exact ``le`` counts at the reference's
``llm_slo_ttft_ms`` boundaries, the count and an exact fixed-point sum.

``SliSketchOracle`` is the rules in numpy: the reference the device sketch (ops/csrc/slisketch.hip,
ops/slisketch.py) is tested against for equality, and what ``engine="cpu"`` uses.

The bucket of a value is read off its float32 image -- no logarithm, so host and device cannot
differ: ``key = (bits & 0x7fffffff) >> 19`` (the exponent and the top 4 mantissa bits: 16 linear
sub-buckets per octave); bucket 0 (underflow) for ``key < LO`` = the key of 0.125 ms (0, -0.0 and
denormals with it), buckets 1..384 = ``key - LO + 1`` (24 octaves up to 2^21 ms), bucket 385
(overflow) above, +inf with it.

A 64-byte SPAN counts when it carries no SPAN_NO_SLI and ``group_id < n_groups`` (what the engine
counts in ``sli`` / ``late``); of those a ``ttft_ms >= 0`` (float compare: NaN and negatives fail)
is observed, the rest is ``invalid`` -- the engine counts such a record as a request within the
SLO, so the sketch's ``n`` can be below ``sli[g][0] + late[g][0]`` by exactly these. SPAN_LATE
records count by their value like any other.

Quantiles are nearest-rank over the buckets: rank ``max(1, (q * n + 999) // 1000)`` for the
per-mille ``q`` of PERMILLE, the first bucket whose inclusive cumulative count reaches it,
published as the bucket's index (EMPTY for a group without a record). ``representative`` maps an
index to ms: the midpoint of the bucket's edges, within a relative 1/32 of every value in it.

The horizon is counted in steps, not in time: every step evicts the step ``windows`` before it,
in every row of ``group_cap``, whether or not the step holds a record or the group is present.
"""

from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

from ..collector import records
from .trackerstate import OracleCheckpoint
from .oracle import milli_units

KEY_SHIFT = 19
LO = (127 - 3) << 4          # key of 0.125 ms
NB = 384                     # 24 octaves x 16
K = NB + 2                   # + underflow (0) and overflow (K - 1)
ROW_STRIDE = 392             # words a histogram row takes on the device (the memory bound's unit)
MAX_MS = float(2 ** 21)
EDGES = (50.0, 100.0, 200.0, 400.0, 800.0, 1200.0, 2000.0)   # REF llm_slo_ttft_ms
N_LE = len(EDGES) + 1
PERMILLE = (500, 900, 950, 990)
QUANTILE_NAMES = ("0.5", "0.9", "0.95", "0.99")
EMPTY = 0xFFFFFFFF
# per-step statistics, in the device's order (ops/csrc/slisketch_host.h Stat)
STATS = ("observed", "invalid", "underflow", "overflow", "out_of_group")
N_STATS = 8
EVENT_STATS = ("invalid", "underflow", "overflow")
RESULT_FIELDS = ("n", "sum_milli", "le", "q_win", "n_roll", "q_roll", "stats")
# what WindowPipeline.results() gains with the sketch on
RESULT_KEYS = ("ttft_n", "ttft_sum_ms", "ttft_le", "ttft_q", "ttft_q_roll", "ttft_n_roll")


def stats_dict(stats: np.ndarray) -> Dict[str, int]:
    return {name: int(stats[i]) for i, name in enumerate(STATS)}


def bucket_of(v) -> np.ndarray:
    """The bucket (0..K-1) of every float32 in ``v`` (int64, ``v``'s shape)."""
    x = np.asarray(v, dtype=np.float32)
    bits = np.ascontiguousarray(x).reshape(-1).view(np.uint32)
    key = ((bits & np.uint32(0x7FFFFFFF)) >> np.uint32(KEY_SHIFT)).astype(np.int64)
    return np.where(key < LO, 0, np.where(key >= LO + NB, K - 1, key - LO + 1)).astype(np.int64).reshape(x.shape)


def bucket_edges() -> np.ndarray:
    """float64 [NB + 1]: ``edges[b - 1]`` is the lower and ``edges[b]`` the upper (exclusive) edge of
    bucket ``b`` in 1..NB; ``edges[0]`` = 0.125, ``edges[NB]`` = 2^21."""
    keys = (np.arange(NB + 1, dtype=np.uint32) + np.uint32(LO)) << np.uint32(KEY_SHIFT)
    return keys.view(np.float32).astype(np.float64)


def representative() -> np.ndarray:
    """float64 [K]: the ms a bucket index stands for (0 for the underflow, 2^21 for the overflow bucket)."""
    e = bucket_edges()
    out = np.zeros(K, dtype=np.float64)
    out[1:NB + 1] = 0.5 * (e[:-1] + e[1:])
    out[K - 1] = MAX_MS
    return out


def _to_ms(q: np.ndarray) -> np.ndarray:
    q = np.asarray(q).astype(np.int64)
    return np.where(q == EMPTY, np.nan, representative()[np.minimum(q, K - 1)])


def quantiles_ms(result: Dict[str, np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    """(window, rolling) quantiles [G, 4] in ms of a step's results; NaN for an empty group."""
    return _to_ms(result["q_win"]), _to_ms(result["q_roll"])


def result_keys(result: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """A step's results under the names WindowPipeline.results() carries (RESULT_KEYS)."""
    qw, qr = quantiles_ms(result)
    return {"ttft_n": np.asarray(result["n"]), "ttft_sum_ms": np.asarray(result["sum_milli"]).astype(np.float64) * 1e-3,
            "ttft_le": np.asarray(result["le"]), "ttft_q": qw, "ttft_q_roll": qr,
            "ttft_n_roll": np.asarray(result["n_roll"])}


def empty_result(n_groups: int) -> Dict[str, np.ndarray]:
    G = int(n_groups)
    return {"n": np.zeros(G, np.uint32), "sum_milli": np.zeros(G, np.uint64), "le": np.zeros((G, N_LE), np.uint32),
            "q_win": np.full((G, len(PERMILLE)), EMPTY, np.uint32), "n_roll": np.zeros(G, np.uint32),
            "q_roll": np.full((G, len(PERMILLE)), EMPTY, np.uint32), "stats": np.zeros(N_STATS, np.uint32)}


def rank_buckets(hist: np.ndarray) -> np.ndarray:
    """uint32 [rows, 4]: per row of ``hist`` [rows, K] the first bucket whose inclusive cumulative
    count reaches each nearest rank; EMPTY for an empty row."""
    cum = np.cumsum(hist.astype(np.int64), axis=1)
    out = np.full((hist.shape[0], len(PERMILLE)), EMPTY, dtype=np.uint32)
    for g in np.nonzero(cum[:, -1] > 0)[0].tolist():
        n = int(cum[g, -1])
        for j, q in enumerate(PERMILLE):
            r = max(1, (q * n + 999) // 1000)
            out[g, j] = int(np.searchsorted(cum[g], r, side="left"))
    return out


def _gather(ranges) -> np.ndarray:
    from .cpu import _gather as g

    b = g(ranges)
    return b.view(records.SPAN) if len(b) else np.zeros(0, records.SPAN)


class SliSketchOracle(OracleCheckpoint):
    """The sketch's rules in numpy (see the module docstring), with the device handle's interface."""

    # checkpoint (pipeline/trackerstate.py): the fields ops/csrc/slisketch_host.h fingerprint() covers, and what is
    # kept between steps
    KIND = "ttft sketch"
    FINGERPRINT = ("group_cap", "windows")
    STATE = ("roll", "held", "last", "n")

    def __init__(self, span_cap: int = 16384, group_cap: int = 64, windows: int = 150, n_buffers: int = 3,
                 device: int = 0):
        span_cap, group_cap, windows, n_buffers = int(span_cap), int(group_cap), int(windows), int(n_buffers)
        if not 1 <= windows <= 4096:
            raise ValueError("ttft sketch: windows must be in [1, 4096]")
        if not 0 < span_cap <= 1 << 24 or span_cap * windows >= 1 << 32:
            raise ValueError("ttft sketch: span_cap out of range (span_cap * windows must stay below 2^32)")
        if not 1 <= group_cap <= 65536:
            raise ValueError("ttft sketch: group_cap must be in [1, 65536]")
        if not 1 <= n_buffers <= 64:
            raise ValueError("ttft sketch: n_buffers out of range")
        if (windows + 2) * group_cap * ROW_STRIDE * 4 > 1 << 31:
            raise ValueError("ttft sketch: the histograms of windows x group_cap need more than 2 GiB")
        self.span_cap, self.group_cap, self.windows, self.nb = span_cap, group_cap, windows, n_buffers
        self.roll = np.zeros((group_cap, K), np.int64)
        self.held: Dict[int, np.ndarray] = {}  # step % windows -> that step's histogram
        self.last = np.zeros((group_cap, K), np.int64)
        self.res: Dict[int, Tuple[int, dict]] = {}
        self.n = 0

    # ---- one window ---------------------------------------------------------------------------
    def step(self, span_ranges: Sequence[Tuple[int, int]], n_groups: int) -> int:
        """``span_ranges`` = [(host address, bytes)] of 64-byte SPAN records, as the engine gets them."""
        for _a, nbytes in span_ranges:
            if int(nbytes) % 64:
                raise ValueError("ttft sketch step: a range is not whole 64-byte spans")
        return self.step_records(_gather(span_ranges), n_groups)

    def step_records(self, spans: np.ndarray, n_groups: int) -> int:
        G, C = int(n_groups), self.group_cap
        if not 0 <= G <= C:
            raise ValueError("ttft sketch step: n_groups out of range")
        if len(spans) > self.span_cap:
            raise ValueError("ttft sketch step: more spans than span_cap")
        grp = spans["group_id"].astype(np.int64)
        v = np.ascontiguousarray(spans["ttft_ms"], dtype=np.float32)
        sli = (spans["flags"] & np.uint32(records.SPAN_NO_SLI)) == 0
        counts = sli & (grp < G)
        with np.errstate(invalid="ignore"):
            ok = counts & (v >= np.float32(0.0))
        g, x = grp[ok], v[ok]
        b = bucket_of(x)
        hist = np.zeros((C, K), np.int64)
        np.add.at(hist, (g, b), 1)
        le = np.zeros((C, N_LE), np.uint32)
        np.add.at(le, (g, (x[:, None] > np.array(EDGES, np.float32)[None, :]).sum(axis=1)), 1)
        sums = np.zeros(C, np.uint64)
        np.add.at(sums, g, milli_units(np.minimum(x, np.float32(MAX_MS))).astype(np.uint64))
        stats = np.zeros(N_STATS, np.uint32)
        stats[:len(STATS)] = [int(ok.sum()), int((counts & ~ok).sum()), int((b == 0).sum()), int((b == K - 1).sum()),
                              int((sli & (grp >= G)).sum())]
        idx = self.n
        slot = idx % self.windows
        self.roll += hist - self.held.get(slot, 0)
        self.held[slot] = hist
        self.last = hist
        res = {"n": hist.sum(axis=1).astype(np.uint32), "sum_milli": sums, "le": le, "q_win": rank_buckets(hist),
               "n_roll": self.roll.sum(axis=1).astype(np.uint32), "q_roll": rank_buckets(self.roll), "stats": stats}
        self.res[idx % self.nb] = (idx, res)
        self.n += 1
        return idx

    # ---- results ------------------------------------------------------------------------------
    def query(self, i: int) -> bool:
        return True

    def results(self, i: int, n_groups: int) -> Dict[str, np.ndarray]:
        held = self.res.get(int(i) % self.nb)
        if held is None or held[0] != int(i):
            raise IndexError(f"ttft sketch step {i} is not held (only the last {self.nb})")
        G = int(n_groups)
        if not 0 <= G <= self.group_cap:
            raise ValueError("n_groups")
        return {k: (v.copy() if k == "stats" else v[:G].copy()) for k, v in held[1].items()}

    def step_ms(self, i: int) -> Tuple[float, float]:
        return 0.0, 0.0

    def rolling(self) -> np.ndarray:
        return self.roll.astype(np.uint32)

    def window_hist(self) -> np.ndarray:
        return self.last.astype(np.uint32)

    def sync(self) -> None:
        pass

    def close(self) -> None:
        pass
