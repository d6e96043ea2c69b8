"""TTFT drift on the host: the rules of the drift tracker (docs/TTFT_DRIFT.md is the contract).

Every decision the agent makes about a service is a function of its breach count, so a fault that moves
a service's TTFT *towards* the SLO without crossing it is invisible. Per step (one window, the span
ranges the engine gets) this tracker decides, per service (incident group), whether the TTFT
distribution of the last ``R`` windows (**recent**) is stochastically slower, or faster, than that of
the last ``B`` calm, non-empty windows that lie at least ``L`` windows further back (**baseline**).

**Which records count, and the bucket** are the TTFT sketch's (pipeline/slisketch.py): no SPAN_NO_SLI
and ``group_id < n_groups``, else ``out_of_group``; ``ttft_ms >= 0`` in float32, else ``invalid``; the
bucket read off the float32 image, K = 386.

**Rings**, per service and step ``i`` (from 0), in this order, in every row of ``group_cap``:

1. ``recent += cur``; if ``i >= R``: ``recent -= near[(i - R) % (R + L)]``.
2. if ``i >= R + L``: ``x = near[i % (R + L)]`` (the window of step ``i - R - L``) leaves the gap. It is
   *admitted* to the baseline iff the service's published state of step ``i - 1`` has no ``slow`` bit
   and ``x`` holds a record: with ``base_fill == B`` the oldest ring row ``base_ring[base_pos % B]``
   leaves ``base``, else ``base_fill += 1``; then ``base += x``, the ring row becomes ``x``,
   ``base_pos += 1``. A non-empty ``x`` that is not admitted is *withheld*.
3. ``near[i % (R + L)] = cur``.

**The statistic**, all in unsigned 64-bit, no division: with ``n_r`` / ``n_b`` the totals and ``C_r(k)``
/ ``C_b(k)`` the inclusive cumulative counts of ``recent`` / ``base``: ``slow_num = max_k (C_b(k) n_r -
C_r(k) n_b)`` clamped at 0, ``fast_num`` its mirror, ``slow_at`` / ``fast_at`` the first bucket that
attains it (EMPTY for 0). ``q_recent`` / ``q_base`` are the sketch's nearest-rank buckets.

**Decision**: with ``n_r >= min_recent``, ``n_b >= min_base`` and ``base_fill >= min_base_windows``:
``Dq = (num << 16) // (n_r n_b)``, ``n_e = (n_r n_b) // (n_r + n_b)``, significant iff ``Dq Dq n_e >
crit_q`` = ``floor(c^2 2^32 + 0.5)``. ``slow`` (bit 0) iff significant and p50 or p90 of recent lies at
least ``s`` buckets above the baseline's; ``fast`` (bit 1) is the mirror image. Otherwise the service
is ``warming`` (bit 2) with no direction bit.

**Hold and reset**: ``hold`` counts consecutive ``slow`` steps; when it reaches ``hold_max`` the
baseline is dropped (``base = 0``, ``base_fill = 0``, ``hold = 0``) and the step's state is ``warming |
rebased`` (bit 3). The step's other fields show the row as it was decided on.

``DriftOracle`` is the rules in numpy: the reference the device tracker (ops/csrc/drift.hip,
ops/drift.py) is tested against for equality, and what ``engine="cpu"`` uses.
"""

from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from ..collector import records
from .trackerstate import OracleCheckpoint
from . import slisketch
from .slisketch import EMPTY, K, PERMILLE, ROW_STRIDE, bucket_of, rank_buckets  # noqa: F401 - the sketch's rules

PER_LANE = 7                 # buckets a lane of the roll kernel's wave owns
SLOW, FAST, WARMING, REBASED = 1, 2, 4, 8
P50, P90 = 0, 1              # of PERMILLE
# per-step statistics, in the device's order (ops/csrc/drift_host.h Stat)
STATS = ("observed", "invalid", "out_of_group", "admitted", "withheld", "rebased")
N_STATS = 8
EVENT_STATS = ("invalid", "out_of_group", "admitted", "withheld", "rebased")
RESULT_FIELDS = ("n_win", "n_recent", "n_base", "base_fill", "q_recent", "q_base", "slow_num", "fast_num", "slow_at",
                 "fast_at", "state", "hold", "stats")
# what WindowPipeline.results() gains with the tracker on
RESULT_KEYS = ("drift_state", "drift_hold", "drift_n_win", "drift_n_recent", "drift_n_base", "drift_base_fill",
               "drift_slow_num", "drift_fast_num", "drift_q_recent", "drift_q_base")
DEFAULT_CRIT = 4.0           # c^2 (reasoned, untuned)
DEFAULT_MIN_SHIFT = 2        # s, buckets: 1/16 of an octave each, about 6 % together
DEFAULT_MIN_RECENT = 30
DEFAULT_MIN_BASE = 100


def defaults(window_ms: float) -> Tuple[int, int, int]:
    """(R, L, B) for a window of ``window_ms``: 10 s recent, 10 s gap, 300 s baseline (reasoned, untuned)."""
    w = max(float(window_ms), 1e-3)
    r = max(1, int(round(10000.0 / w)))
    return r, r, max(1, int(round(300000.0 / w)))


def crit_q(c2: float) -> int:
    x = math.floor(float(c2) * 4294967296.0 + 0.5)
    return int(min(max(x, 0), (1 << 64) - 1))


def stats_dict(stats: np.ndarray) -> Dict[str, int]:
    return {name: int(stats[i]) for i, name in enumerate(STATS)}


def state_name(state: int) -> str:
    s = int(state)
    return "rebased" if s & REBASED else "warming" if s & WARMING else "slow" if s & SLOW else "fast" if s & FAST else "calm"


def result_keys(result: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """A step's results under the names WindowPipeline.results() carries (RESULT_KEYS)."""
    return {"drift_" + k: np.asarray(result[k]) for k in ("state", "hold", "n_win", "n_recent", "n_base", "base_fill",
                                                         "slow_num", "fast_num", "q_recent", "q_base")}


def empty_result(n_groups: int) -> Dict[str, np.ndarray]:
    G = int(n_groups)
    z = lambda: np.zeros(G, np.uint32)  # noqa: E731
    return {"n_win": z(), "n_recent": z(), "n_base": z(), "base_fill": z(),
            "q_recent": np.full((G, len(PERMILLE)), EMPTY, np.uint32), "q_base": np.full((G, len(PERMILLE)), EMPTY, np.uint32),
            "slow_num": np.zeros(G, np.uint64), "fast_num": np.zeros(G, np.uint64),
            "slow_at": np.full(G, EMPTY, np.uint32), "fast_at": np.full(G, EMPTY, np.uint32),
            "state": np.full(G, WARMING, np.uint32), "hold": z(), "stats": np.zeros(N_STATS, np.uint32)}


def _ms(q) -> Optional[float]:
    q = int(q)
    return None if q == EMPTY else round(float(slisketch.representative()[min(q, K - 1)]), 4)


def summary(state, hold, n_recent, n_base, slow_num, q_recent, q_base) -> Dict[str, object]:
    """One service's row as the decision log carries it: the state's name, the one-sided KS distance
    ``slow_num / (n_r n_b)``, p50 / p90 in ms as [base, recent] (``None`` for an empty row) and their ratio."""
    nr, nb = int(n_recent), int(n_base)
    p50 = [_ms(q_base[P50]), _ms(q_recent[P50])]
    p90 = [_ms(q_base[P90]), _ms(q_recent[P90])]
    ratio = None if p50[0] is None or p50[1] is None or p50[0] <= 0 else round(p50[1] / p50[0], 6)
    return {"state": state_name(state), "distance": None if nr == 0 or nb == 0 else round(int(slow_num) / (nr * nb), 6),
            "n_recent": nr, "n_base": nb, "p50_ms": p50, "p90_ms": p90, "shift_ratio": ratio, "held_windows": int(hold)}


def decide(n_r: int, n_b: int, base_fill: int, slow_num: int, fast_num: int, q_recent, q_base, crit: int, min_shift: int,
           min_recent: int, min_base: int, min_base_windows: int) -> int:
    """The state bits of one service before hold and reset (ops/csrc/drift_host.h ``decide``); ``crit`` is crit_q."""
    n_r, n_b = int(n_r), int(n_b)
    if n_r == 0 or n_b == 0 or n_r < min_recent or n_b < min_base or int(base_fill) < min_base_windows:
        return WARMING
    nn, ne = n_r * n_b, (n_r * n_b) // (n_r + n_b)

    def sig(num: int) -> bool:
        dq = (int(num) << 16) // nn
        return dq * dq * ne > crit

    qr, qb, s = [int(x) for x in q_recent], [int(x) for x in q_base], int(min_shift)
    st = 0
    if sig(slow_num) and (qr[P50] >= qb[P50] + s or qr[P90] >= qb[P90] + s):
        st |= SLOW
    if sig(fast_num) and (qb[P50] >= qr[P50] + s or qb[P90] >= qr[P90] + s):
        st |= FAST
    return st


# ---- layout and checks (ops/csrc/drift_host.h) ----------------------------------------------------
def layout(group_cap: int) -> Dict[str, int]:
    """Word offsets of the result block's arrays (every array on 16 bytes) and its ``words``."""
    g = int(group_cap)
    one, pair = (g + 3) & ~3, (2 * g + 3) & ~3
    off, at = {}, 0
    for name, n in (("n_win", one), ("n_recent", one), ("n_base", one), ("base_fill", one), ("q_recent", 4 * g),
                    ("q_base", 4 * g), ("slow_num", pair), ("fast_num", pair), ("slow_at", one), ("fast_at", one),
                    ("state", one), ("hold", one), ("stats", N_STATS)):
        off[name] = at
        at += n
    off["words"] = at
    return off


def device_bytes(span_cap: int, group_cap: int, recent: int, gap: int, baseline: int) -> int:
    return ((int(recent) + int(gap) + int(baseline) + 3) * int(group_cap) * ROW_STRIDE * 4 + int(span_cap) * 64
            + layout(group_cap)["words"] * 4)


def check_config(span_cap: int, group_cap: int, recent: int, gap: int, baseline: int, n_buffers: int, crit: float,
                 min_shift: int, min_recent: int, min_base: int, min_base_windows: int, hold_max: int) -> None:
    """The configuration checks of ops/csrc/drift_host.h validate()."""
    if not 1 <= recent <= 1024:
        raise ValueError("ttft drift: recent windows must be in [1, 1024]")
    if not 1 <= gap <= 1024:
        raise ValueError("ttft drift: gap windows must be in [1, 1024]")
    if not 1 <= baseline <= 4096:
        raise ValueError("ttft drift: baseline windows must be in [1, 4096]")
    if not 1 <= group_cap <= 65536:
        raise ValueError("ttft drift: group_cap must be in [1, 65536]")
    if span_cap < 1:
        raise ValueError("ttft drift: span_cap must be >= 1")
    if span_cap * span_cap * recent * baseline >= 1 << 44:
        raise ValueError("ttft drift: span_cap^2 * recent * baseline must stay below 2^44 (slow_num << 16 would wrap)")
    if not 1 <= n_buffers <= 64:
        raise ValueError("ttft drift: n_buffers out of range")
    if not (np.isfinite(crit) and crit > 0):
        raise ValueError("ttft drift: crit must be finite and > 0")
    if not 0 <= min_shift <= K - 1:
        raise ValueError("ttft drift: min_shift must be in [0, 385]")
    if not (1 <= min_recent <= 0xFFFFFFFF and 1 <= min_base <= 0xFFFFFFFF and min_base_windows >= 1):
        raise ValueError("ttft drift: min_recent, min_base and min_base_windows must be >= 1")
    if not 1 <= hold_max <= 0xFFFFFFFF:
        raise ValueError("ttft drift: hold_max must be >= 1")
    if device_bytes(span_cap, group_cap, recent, gap, baseline) > 1 << 31:
        raise ValueError("ttft drift: the rings need more than 2 GiB")


def resolve(recent: int, gap: int, baseline: int, crit: Optional[float], min_shift: Optional[int],
            min_recent: Optional[int], min_base: Optional[int], min_base_windows: Optional[int],
            hold_max: Optional[int]) -> Dict[str, object]:
    """The configuration with every ``None`` replaced by its default (``min_base_windows = min(B, 10)``,
    ``hold_max = 4 B``)."""
    B = int(baseline)
    return {"recent": int(recent), "gap": int(gap), "baseline": B,
            "crit": DEFAULT_CRIT if crit is None else float(crit),
            "min_shift": DEFAULT_MIN_SHIFT if min_shift is None else int(min_shift),
            "min_recent": DEFAULT_MIN_RECENT if min_recent is None else int(min_recent),
            "min_base": DEFAULT_MIN_BASE if min_base is None else int(min_base),
            "min_base_windows": max(1, min(B, 10)) if min_base_windows is None else int(min_base_windows),
            "hold_max": max(1, 4 * B) if hold_max is None else int(hold_max)}


def block_of(result: Dict[str, np.ndarray], group_cap: int) -> np.ndarray:
    """A step's results over all ``group_cap`` rows as the device's result block (uint32 words)."""
    off = layout(group_cap)
    out = np.zeros(off["words"], np.uint32)
    for name in RESULT_FIELDS:
        a = np.ascontiguousarray(result[name])
        w = a.view(np.uint32).reshape(-1)
        out[off[name]:off[name] + len(w)] = w
    return out


def _gather(ranges) -> np.ndarray:
    from .cpu import _gather as g

    b = g(ranges)
    return b.view(records.SPAN) if len(b) else np.zeros(0, records.SPAN)


def statistic(recent: np.ndarray, base: np.ndarray):
    """(slow_num, fast_num uint64 [G]; slow_at, fast_at uint32 [G]) of the rows ``recent`` / ``base`` [G, K]."""
    cr = np.cumsum(recent.astype(np.int64), axis=1)
    cb = np.cumsum(base.astype(np.int64), axis=1)
    d = cb * cr[:, -1:] - cr * cb[:, -1:]   # below 2^44 in magnitude (check_config)
    out = []
    for e in (d, -d):
        at = np.argmax(e, axis=1)            # the first bucket that attains the maximum
        num = np.maximum(e[np.arange(len(e)), at], 0)
        out.append((num.astype(np.uint64), np.where(num > 0, at, EMPTY).astype(np.uint32)))
    return out[0][0], out[1][0], out[0][1], out[1][1]


class DriftOracle(OracleCheckpoint):
    """The tracker's rules in numpy (see the module docstring), with the device handle's interface."""

    # checkpoint (pipeline/trackerstate.py): the fields ops/csrc/drift_host.h fingerprint() covers, and what is
    # kept between steps
    KIND = "ttft drift"
    FINGERPRINT = ("group_cap", "cfg")
    STATE = ("near", "recent", "base_ring", "base", "base_fill", "base_pos", "hold", "prev", "n")

    def __init__(self, span_cap: int = 16384, group_cap: int = 64, recent: int = 10, gap: int = 10, baseline: int = 300,
                 n_buffers: int = 3, crit: Optional[float] = None, min_shift: Optional[int] = None,
                 min_recent: Optional[int] = None, min_base: Optional[int] = None,
                 min_base_windows: Optional[int] = None, hold_max: Optional[int] = None, device: int = 0,
                 lds: bool = True):
        span_cap, group_cap, n_buffers = int(span_cap), int(group_cap), int(n_buffers)
        self.cfg = resolve(recent, gap, baseline, crit, min_shift, min_recent, min_base, min_base_windows, hold_max)
        check_config(span_cap, group_cap, n_buffers=n_buffers, **self.cfg)
        self.span_cap, self.group_cap, self.nb = span_cap, group_cap, n_buffers
        self.R, self.L, self.B = self.cfg["recent"], self.cfg["gap"], self.cfg["baseline"]
        self.crit_q = crit_q(self.cfg["crit"])
        C = group_cap
        self.near = np.zeros((self.R + self.L, C, K), np.int64)
        self.recent = np.zeros((C, K), np.int64)
        self.base_ring = np.zeros((self.B, C, K), np.int64)
        self.base = np.zeros((C, K), np.int64)
        self.base_fill = np.zeros(C, np.int64)
        self.base_pos = np.zeros(C, np.int64)
        self.hold = np.zeros(C, np.int64)
        self.prev = np.zeros(C, np.int64)   # the published state of the step before
        self.res: Dict[int, Tuple[int, dict]] = {}
        self.n = 0

    # ---- one window ---------------------------------------------------------------------------
    def step(self, span_ranges: Sequence[Tuple[int, int]], n_groups: int) -> int:
        """``span_ranges`` = [(host address, bytes)] of 64-byte SPAN records, as the engine gets them."""
        for a, nbytes in span_ranges:
            if int(nbytes) % 64:
                raise ValueError("ttft drift step: a range is not whole 64-byte spans")
            if int(nbytes) and not int(a):
                raise ValueError("ttft drift step: null range")
        return self.step_records(_gather(span_ranges), n_groups)

    def step_records(self, spans: np.ndarray, n_groups: int) -> int:
        G, C = int(n_groups), self.group_cap
        if not 0 <= G <= C:
            raise ValueError("ttft drift step: n_groups out of range")
        if len(spans) > self.span_cap:
            raise ValueError("ttft drift step: more spans than span_cap")
        # nothing has changed up to here
        grp = spans["group_id"].astype(np.int64)
        v = np.ascontiguousarray(spans["ttft_ms"], dtype=np.float32)
        sli = (spans["flags"] & np.uint32(records.SPAN_NO_SLI)) == 0
        counts = sli & (grp < G)
        with np.errstate(invalid="ignore"):
            ok = counts & (v >= np.float32(0.0))
        cur = np.zeros((C, K), np.int64)
        np.add.at(cur, (grp[ok], bucket_of(v[ok])), 1)
        i, R, near, B = self.n, self.R, self.R + self.L, self.B
        c = self.cfg
        # 1. recent
        self.recent += cur
        if i >= R:
            self.recent -= self.near[(i - R) % near]
        # 2. the window that leaves the gap
        admitted = withheld = rebased = 0
        if i >= near:
            x = self.near[i % near]
            for g in np.nonzero(x.sum(axis=1) > 0)[0].tolist():
                if self.prev[g] & SLOW:
                    withheld += 1
                    continue
                at = int(self.base_pos[g] % B)
                if self.base_fill[g] == B:
                    self.base[g] -= self.base_ring[at, g]
                else:
                    self.base_fill[g] += 1
                self.base[g] += x[g]
                self.base_ring[at, g] = x[g]
                self.base_pos[g] += 1
                admitted += 1
        # 3. the near ring
        self.near[i % near] = cur
        # the statistic and the decision
        slow_num, fast_num, slow_at, fast_at = statistic(self.recent, self.base)
        q_r, q_b = rank_buckets(self.recent), rank_buckets(self.base)
        n_r, n_b = self.recent.sum(axis=1), self.base.sum(axis=1)
        fill = self.base_fill.copy()
        state = np.zeros(C, np.uint32)
        for g in range(C):
            st = decide(n_r[g], n_b[g], fill[g], slow_num[g], fast_num[g], q_r[g], q_b[g], self.crit_q, c["min_shift"],
                        c["min_recent"], c["min_base"], c["min_base_windows"])
            self.hold[g] = self.hold[g] + 1 if st & SLOW else 0
            if self.hold[g] >= c["hold_max"]:
                st = WARMING | REBASED
                self.hold[g] = 0
                self.base[g] = 0
                self.base_fill[g] = 0
                rebased += 1
            state[g] = st
        self.prev = state.astype(np.int64)
        stats = np.zeros(N_STATS, np.uint32)
        stats[:len(STATS)] = [int(ok.sum()), int((counts & ~ok).sum()), int((sli & (grp >= G)).sum()), admitted, withheld,
                              rebased]
        res = {"n_win": cur.sum(axis=1).astype(np.uint32), "n_recent": n_r.astype(np.uint32), "n_base": n_b.astype(np.uint32),
               "base_fill": fill.astype(np.uint32), "q_recent": q_r, "q_base": q_b, "slow_num": slow_num, "fast_num": fast_num,
               "slow_at": slow_at, "fast_at": fast_at, "state": state, "hold": self.hold.astype(np.uint32), "stats": stats}
        self.res[i % self.nb] = (i, res)
        self.n += 1
        return i

    # ---- results ------------------------------------------------------------------------------
    def query(self, i: int) -> bool:
        return True

    def _held(self, i: int) -> dict:
        held = self.res.get(int(i) % self.nb)
        if held is None or held[0] != int(i):
            raise IndexError(f"ttft drift step {i} is not held (only the last {self.nb})")
        return held[1]

    def results(self, i: int, n_groups: int) -> Dict[str, np.ndarray]:
        res = self._held(i)
        G = int(n_groups)
        if not 0 <= G <= self.group_cap:
            raise ValueError("n_groups")
        return {k: (v.copy() if k == "stats" else v[:G].copy()) for k, v in res.items()}

    def block(self, i: int) -> np.ndarray:
        """Step ``i``'s results as the device's whole result block (uint32 words)."""
        return block_of(self._held(i), self.group_cap)

    def step_ms(self, i: int) -> Tuple[float, float]:
        return 0.0, 0.0

    def observe_ms(self, i: int) -> float:
        return 0.0

    def resident(self) -> Dict[str, np.ndarray]:
        """The rolling state: ``recent`` / ``base`` [group_cap, ROW_STRIDE], ``base_fill`` / ``base_pos`` / ``hold``
        [group_cap] and ``pos``, the near-ring row the next step replaces."""
        def rows(a):
            out = np.zeros((self.group_cap, ROW_STRIDE), np.uint32)
            out[:, :K] = a
            return out

        return {"recent": rows(self.recent), "base": rows(self.base), "base_fill": self.base_fill.astype(np.uint32),
                "base_pos": self.base_pos.astype(np.uint32), "hold": self.hold.astype(np.uint32),
                "pos": self.n % (self.R + self.L)}

    def sync(self) -> None:
        pass

    def close(self) -> None:
        pass
