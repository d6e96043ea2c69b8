"""Error SLI on the host: the rules of the error SLI tracker.

Every other SLI is a latency. A request that **failed** -- a 429 or a 503 answered in 20 ms -- breaches
none of them. Per step (one window, the span ranges the engine gets) this tracker yields, per service
(incident group): the finished requests by outcome class, for the window and for the last ``windows``
steps (the rolling horizon), and a multi-window, multi-burn-rate evaluation of the availability error
budget: which of up to four (long window, short window, factor) pairs fire, and for how many
consecutive windows something has fired. Everything is in integers.

**The value**: a 64-byte SPAN carries its request's outcome class in bits 4-7 of ``flags``
(``c = (flags >> 4) & 15``, collector/records.py ``span_outcome``): CLASSES[c] for c < 8, 8-15 reserved.
0 = ok is also what every record carries with the feature off.

**Which records count**, checked in this order: a record with SPAN_START or SPAN_FIRST_TOKEN is
skipped silently; ``group_id >= n_groups`` is counted in ``out_of_group``; ``c >= 8`` in ``reserved``;
anything else is observed, ``counts[g][c] += 1``. SPAN_NO_SLI, SPAN_LATE, the TPOT bits and ``ttft_ms``
do not matter. ``n[g]`` is the sum over the 8 classes, ``bad[g]`` the sum over the classes in
``bad_mask`` (default 0xF8: throttled, timeout, unavailable, server, other; client and cancelled are the
caller's).

**Horizon**: counted in steps; every step evicts the step ``windows`` before it, in every row of
``group_cap``.

**Budget and pairs**: ``budget_ppm = clamp(int((1 - target) * 1e6 + 0.5), 1, 10^6)``. Pair p is
``(L, S, factor_milli)`` with ``1 <= S <= L <= windows``. A window X of a pair **burns** iff
``n_X >= min_requests`` and ``n_X > 0`` and ``bad_X * 10^9 >= factor_milli * budget_ppm * n_X``, where
``n_X`` and ``bad_X`` are summed over the last X steps (fewer while the ring fills); equality burns. The
sums are kept rolling: the entering row is added, the row of X steps ago subtracted. A pair **fires**
iff its long and its short window both burn; ``firing[g]`` is the bitmask over pairs; ``age[g]`` the
consecutive steps, this one included, with ``firing[g] != 0``, saturating at 2^32 - 1.
``factor_milli * budget_ppm <= 10^9`` (more would ask for more failures than requests) and
``span_cap * windows < 2^32`` keep both sides of the compare below 2^63.

``ErrorSliOracle`` is the rules in numpy: the reference the device tracker (ops/csrc/errsli.hip,
ops/errsli.py) is tested against for equality, and what ``engine="cpu"`` uses.
"""

from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ..collector import records
from .trackerstate import OracleCheckpoint

CLASSES = ("ok", "client", "cancelled", "throttled", "timeout", "unavailable", "server", "other")
N_CLASSES = 8
MAX_PAIRS = 4
PAIR_WORDS = 4               # n_long, bad_long, n_short, bad_short
BAD_ALLOWED = 0xFE
BAD_DEFAULT = 0xF8
BURN_SCALE = 10 ** 9
MAX_WINDOWS = 32768
SKIP = records.SPAN_START | records.SPAN_FIRST_TOKEN
# per-step statistics, in the device's order (ops/csrc/errsli_host.h Stat)
STATS = ("observed", "out_of_group", "reserved")
N_STATS = 8
EVENT_STATS = ("out_of_group", "reserved")
RESULT_FIELDS = ("counts", "counts_roll", "pair_sums", "firing", "age", "stats")
# what WindowPipeline.results() gains with the tracker on
RESULT_KEYS = ("err_counts", "err_counts_roll", "err_pair_sums", "err_firing", "err_age")
DEFAULT_PAIRS = ((3600, 300, 14400),)
# the SRE workbook's two paging pairs, in seconds: 2 % of a 30-day budget in 1 h, 5 % in 6 h
DEFAULT_PAIRS_S = "3600:300:14.4,21600:1800:6"
DEFAULT_BAD_CLASSES = "throttled,timeout,unavailable,server,other"

Pair = Tuple[int, int, int]


def stats_dict(stats: np.ndarray) -> Dict[str, int]:
    return {name: int(stats[i]) for i, name in enumerate(STATS)}


def budget_ppm(target: float) -> int:
    return int(min(10 ** 6, max(1, int((1.0 - float(target)) * 1e6 + 0.5))))


def burns(n: int, bad: int, min_requests: int, thr: int) -> bool:
    """The burn compare on Python integers (``thr`` = factor_milli * budget_ppm)."""
    return n >= min_requests and n > 0 and bad * BURN_SCALE >= thr * n


def bad_mask_of(names: str) -> int:
    """``"throttled,server"`` -> the mask of those classes; ``ok`` and unknown names are refused."""
    mask = 0
    for name in (x.strip().lower() for x in str(names).split(",")):
        if not name:
            continue
        if name not in CLASSES or name == "ok":
            raise ValueError(f"error sli: {name!r} is no class that can burn the budget "
                             f"(one of {', '.join(CLASSES[1:])})")
        mask |= 1 << CLASSES.index(name)
    if not mask:
        raise ValueError("error sli: no class burns the budget")
    return mask


def parse_pairs(text: str, window_ms: float) -> List[Pair]:
    """``"long_s:short_s:factor,..."`` as (L, S, factor_milli) in windows of ``window_ms``:
    ``ceil(seconds * 1000 / window_ms)``, at least 1. A pair beyond MAX_WINDOWS windows is refused by
    name."""
    out: List[Pair] = []
    for item in (x.strip() for x in str(text).split(",")):
        if not item:
            continue
        parts = item.split(":")
        try:
            if len(parts) != 3:
                raise ValueError
            ls, ss, f = float(parts[0]), float(parts[1]), float(parts[2])
            if not (math.isfinite(ls) and math.isfinite(ss) and math.isfinite(f)):
                raise ValueError
        except ValueError:
            raise ValueError(f"error sli: burn pair {item!r} is not long_s:short_s:factor") from None
        if not (ls > 0 and ss > 0 and ss <= ls and f > 0):
            raise ValueError(f"error sli: burn pair {item!r} needs 0 < short_s <= long_s and a factor > 0")
        L = max(1, int(math.ceil(ls * 1000.0 / float(window_ms))))
        S = max(1, int(math.ceil(ss * 1000.0 / float(window_ms))))
        if L > MAX_WINDOWS:
            raise ValueError(f"error sli: burn pair {item!r} spans {L} windows of {window_ms:g} ms, more than "
                             f"{MAX_WINDOWS}: use a longer --window-ms or a shorter pair")
        out.append((L, S, max(1, int(f * 1000.0 + 0.5))))
    if not 1 <= len(out) <= MAX_PAIRS:
        raise ValueError("error sli: 1 to 4 burn pairs")
    return out


def burn_rate(n: int, bad: int, budget: int) -> Optional[float]:
    """The budget multiples a window of ``n`` requests spends, ``None`` without a request."""
    return None if n == 0 else round((bad / n) / (budget * 1e-6), 6)


def class_summary(counts, bad_mask: int) -> Dict[str, object]:
    c = [int(x) for x in counts]
    n = sum(c)
    bad = sum(x for j, x in enumerate(c) if (bad_mask >> j) & 1)
    return {"requests": n, "bad": bad, "ratio": None if n == 0 else round(bad / n, 6),
            "by_class": {name: c[j] for j, name in enumerate(CLASSES)}}


def summary(res: dict, g: int, pairs: Sequence[Pair], budget: int, bad_mask: int) -> Dict[str, object]:
    """Group g's error SLI as the decision log carries it, from the ``err_*`` keys."""
    sums = np.asarray(res["err_pair_sums"][g], dtype=np.int64)
    firing = int(res["err_firing"][g])
    burn = [{"long_windows": int(L), "short_windows": int(S), "factor": f / 1000.0,
             "long": burn_rate(int(sums[p, 0]), int(sums[p, 1]), budget),
             "short": burn_rate(int(sums[p, 2]), int(sums[p, 3]), budget), "firing": bool((firing >> p) & 1)}
            for p, (L, S, f) in enumerate(pairs)]
    return {**class_summary(res["err_counts"][g], bad_mask), "horizon": class_summary(res["err_counts_roll"][g], bad_mask),
            "burn": burn, "firing": firing, "age_windows": int(res["err_age"][g])}


def result_keys(result: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """A step's results under the names WindowPipeline.results() carries (RESULT_KEYS)."""
    return {"err_counts": np.asarray(result["counts"]), "err_counts_roll": np.asarray(result["counts_roll"]),
            "err_pair_sums": np.asarray(result["pair_sums"]), "err_firing": np.asarray(result["firing"]),
            "err_age": np.asarray(result["age"])}


def empty_result(n_groups: int) -> Dict[str, np.ndarray]:
    G = int(n_groups)
    return {"counts": np.zeros((G, N_CLASSES), np.uint32), "counts_roll": np.zeros((G, N_CLASSES), np.uint32),
            "pair_sums": np.zeros((G, MAX_PAIRS, PAIR_WORDS), np.uint32), "firing": np.zeros(G, np.uint32),
            "age": np.zeros(G, np.uint32), "stats": np.zeros(N_STATS, np.uint32)}


# ---- layout and checks (ops/csrc/errsli_host.h) ---------------------------------------------------
def layout(group_cap: int) -> Dict[str, int]:
    """Word offsets of the result block's arrays (every array on 16 bytes) and its ``words``."""
    g = int(group_cap)
    one = (g + 3) & ~3
    off, at = {}, 0
    for name, n in (("counts", 8 * g), ("counts_roll", 8 * g), ("pair_sums", 16 * g), ("firing", one), ("age", one),
                    ("stats", N_STATS)):
        off[name] = at
        at += n
    off["words"] = at
    return off


def device_bytes(span_cap: int, group_cap: int, windows: int) -> int:
    return (int(span_cap) * 64 + (int(windows) + 2) * int(group_cap) * N_CLASSES * 4
            + int(group_cap) * (MAX_PAIRS * PAIR_WORDS + 1) * 4 + layout(group_cap)["words"] * 4)


def check_config(span_cap: int, group_cap: int, windows: int, n_buffers: int, target: float, pairs: Sequence[Pair],
                 min_requests: int, bad_mask: int) -> None:
    """The configuration checks of ops/csrc/errsli_host.h validate()."""
    if not 1 <= windows <= MAX_WINDOWS:
        raise ValueError("error sli: windows must be in [1, 32768]")
    if not 1 <= group_cap <= 65536:
        raise ValueError("error sli: group_cap must be in [1, 65536]")
    if span_cap < 1:
        raise ValueError("error sli: span_cap must be >= 1")
    if span_cap * windows >= 1 << 32:
        raise ValueError("error sli: span_cap * windows must stay below 2^32 (a rolling counter would wrap)")
    if not 1 <= n_buffers <= 64:
        raise ValueError("error sli: n_buffers out of range")
    if not (math.isfinite(target) and 0.0 <= target < 1.0):
        raise ValueError("error sli: target must be finite and in [0, 1)")
    if not 1 <= len(pairs) <= MAX_PAIRS:
        raise ValueError("error sli: 1 to 4 burn pairs")
    budget = budget_ppm(target)
    for L, S, f in pairs:
        if not 1 <= S <= L <= windows:
            raise ValueError("error sli: a pair needs 1 <= short <= long <= windows")
        if f < 1:
            raise ValueError("error sli: a pair's factor_milli must be >= 1")
        if f * budget > BURN_SCALE:
            raise ValueError("error sli: factor * budget above 1 asks for more failures than requests")
    if not 0 <= min_requests < 1 << 32:
        raise ValueError("error sli: min_requests must be in [0, 2^32)")
    if bad_mask == 0 or bad_mask & ~BAD_ALLOWED:
        raise ValueError("error sli: bad_mask must be non-zero and within 0xFE")
    if device_bytes(span_cap, group_cap, windows) > 1 << 31:
        raise ValueError("error sli: the horizon needs more than 2 GiB")


def _pairs(pairs) -> List[Pair]:
    out = []
    for p in pairs:
        L, S, f = p
        if int(L) != L or int(S) != S or int(f) != f:
            raise ValueError("error sli: a pair is (long windows, short windows, factor_milli), integers")
        out.append((int(L), int(S), int(f)))
    return out


def block_of(result: Dict[str, np.ndarray], group_cap: int) -> np.ndarray:
    """A step's results over all ``group_cap`` rows as the device's result block (uint32 words)."""
    off = layout(group_cap)
    out = np.zeros(off["words"], np.uint32)
    for name in RESULT_FIELDS:
        w = np.ascontiguousarray(result[name]).view(np.uint32).reshape(-1)
        out[off[name]:off[name] + len(w)] = w
    return out


def _gather(ranges) -> np.ndarray:
    from .cpu import _gather as g

    b = g(ranges)
    return b.view(records.SPAN) if len(b) else np.zeros(0, records.SPAN)


class ErrorSliOracle(OracleCheckpoint):
    """The tracker's rules in numpy (see the module docstring), with the device handle's interface."""

    # checkpoint (pipeline/trackerstate.py): the fields ops/csrc/errsli_host.h fingerprint() covers, and what is
    # kept between steps
    KIND = "error sli"
    FINGERPRINT = ("group_cap", "windows", "target", "pairs", "min_requests", "bad_mask")
    STATE = ("ring", "roll", "sums", "age", "n")

    def __init__(self, span_cap: int = 16384, group_cap: int = 64, windows: int = 3600, n_buffers: int = 3,
                 target: float = 0.999, pairs: Sequence[Pair] = DEFAULT_PAIRS, min_requests: int = 20,
                 bad_mask: int = BAD_DEFAULT, device: int = 0, lds: bool = True):
        span_cap, group_cap, windows, n_buffers = int(span_cap), int(group_cap), int(windows), int(n_buffers)
        pairs = _pairs(pairs)
        check_config(span_cap, group_cap, windows, n_buffers, float(target), pairs, int(min_requests), int(bad_mask))
        self.span_cap, self.group_cap, self.windows, self.nb = span_cap, group_cap, windows, n_buffers
        self.target, self.pairs, self.min_requests, self.bad_mask = float(target), pairs, int(min_requests), int(bad_mask)
        self.budget_ppm = budget_ppm(target)
        self.bad_cols = np.array([(self.bad_mask >> j) & 1 for j in range(N_CLASSES)], bool)
        self.ring = np.zeros((windows, group_cap, N_CLASSES), np.uint32)   # calloc: untouched rows cost nothing
        self.roll = np.zeros((group_cap, N_CLASSES), np.int64)
        self.sums = np.zeros((group_cap, MAX_PAIRS, PAIR_WORDS), np.int64)
        self.age = np.zeros(group_cap, np.int64)
        self.res: Dict[int, Tuple[int, dict]] = {}
        self.n = 0

    # ---- one window ---------------------------------------------------------------------------
    def step(self, span_ranges: Sequence[Tuple[int, int]], n_groups: int) -> int:
        """``span_ranges`` = [(host address, bytes)] of 64-byte SPAN records, as the engine gets them."""
        for a, nbytes in span_ranges:
            if int(nbytes) % 64:
                raise ValueError("error sli step: a range is not whole 64-byte spans")
            if int(nbytes) and not int(a):
                raise ValueError("error sli step: null range")
        return self.step_records(_gather(span_ranges), n_groups)

    def _n_bad(self, row: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        r = row.astype(np.int64)
        return r.sum(axis=1), r[:, self.bad_cols].sum(axis=1)

    def step_records(self, spans: np.ndarray, n_groups: int) -> int:
        G, C = int(n_groups), self.group_cap
        if not 0 <= G <= C:
            raise ValueError("error sli step: n_groups out of range")
        if len(spans) > self.span_cap:
            raise ValueError("error sli step: more spans than span_cap")
        # nothing has changed up to here
        fl = spans["flags"].astype(np.uint32)
        grp = spans["group_id"].astype(np.int64)
        c = records.span_outcome(fl).astype(np.int64)
        final = (fl & np.uint32(SKIP)) == 0
        ingrp = final & (grp < G)
        ok = ingrp & (c < N_CLASSES)
        counts = np.zeros((C, N_CLASSES), np.int64)
        np.add.at(counts, (grp[ok], c[ok]), 1)
        stats = np.zeros(N_STATS, np.uint32)
        stats[:len(STATS)] = [int(ok.sum()), int((final & ~ingrp).sum()), int((ingrp & ~ok).sum())]
        idx = self.n
        W = self.windows
        en, eb = self._n_bad(counts)
        fire = np.zeros(C, np.int64)
        for p, (L, S, f) in enumerate(self.pairs):
            thr = np.uint64(f * self.budget_ppm)
            both = np.ones(C, bool)
            for k, X in enumerate((L, S)):
                # the row that leaves this window is read before the entering row takes its slot (X == W)
                ln, lb = self._n_bad(self.ring[(idx - X) % W]) if idx >= X else (0, 0)
                self.sums[:, p, 2 * k] += en - ln
                self.sums[:, p, 2 * k + 1] += eb - lb
                n = self.sums[:, p, 2 * k].astype(np.uint64)
                bad = self.sums[:, p, 2 * k + 1].astype(np.uint64)
                both &= (n >= np.uint64(self.min_requests)) & (n > 0) & (bad * np.uint64(BURN_SCALE) >= thr * n)
            fire |= both.astype(np.int64) << p
        slot = idx % W
        self.roll += counts - self.ring[slot].astype(np.int64)
        self.ring[slot] = counts.astype(np.uint32)
        self.age = np.where(fire != 0, np.minimum(self.age + 1, 0xFFFFFFFF), 0)
        res = {"counts": counts.astype(np.uint32), "counts_roll": self.roll.astype(np.uint32),
               "pair_sums": self.sums.astype(np.uint32), "firing": fire.astype(np.uint32),
               "age": self.age.astype(np.uint32), "stats": stats}
        self.res[idx % self.nb] = (idx, res)
        self.n += 1
        return idx

    # ---- results ------------------------------------------------------------------------------
    def query(self, i: int) -> bool:
        return True

    def _held(self, i: int) -> dict:
        held = self.res.get(int(i) % self.nb)
        if held is None or held[0] != int(i):
            raise IndexError(f"error sli step {i} is not held (only the last {self.nb})")
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
        """The rolling state: ``counts`` [group_cap, 8], ``pair_sums`` [group_cap, 4, 4], ``age``
        [group_cap] and ``pos``, the horizon row the next step replaces."""
        return {"counts": self.roll.astype(np.uint32), "pair_sums": self.sums.astype(np.uint32),
                "age": self.age.astype(np.uint32), "pos": self.n % self.windows}

    def sync(self) -> None:
        pass

    def close(self) -> None:
        pass
