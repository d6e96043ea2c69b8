"""Saturation curve per service on the host: the rules of the saturation tracker.

The load tracker says whether load went up; nothing relates load to latency. This tracker keeps, per
service, requests and TTFT breaches by the concurrency of the time bin the request arrived in. From that
curve it finds the concurrency above which the TTFT SLO's error budget is exceeded -- the **knee** -- and
compares the service's recent concurrency with it. Everything is in integers: device and oracle are
compared for equality.

**Records**: the load tracker's checks in its order (pipeline/loadsli.py): SPAN_START or
SPAN_FIRST_TOKEN: skipped; ``group_id >= n_groups``: ``out_of_group``; ``latency_ms`` NaN, ``< 0`` or
above a day: ``invalid``; ``ts_ns <= 0``: ``no_time``; else ``observed``. Its placement decides where a
record's start and end go and the ``future``, ``too_old`` and ``clipped`` counts. An observed record with
``not (ttft_ms >= 0)`` is ``no_ttft``: it still occupies its interval, but it does not enter the curve.

**Cells**: per (service, slot) the load tracker's ``counts`` and ``idle_us`` and a third u64 cell
``sli``: requests with a TTFT in the low word, those with ``ttft_ms > slo_ms`` (float32) in the high one.
Wherever a **start** is placed a record with a TTFT adds ``1 + (breach << 32)`` there; a clipped record
adds nothing to ``sli``.

**A bin's level**: with ``A`` the requests in flight before the bin, ``active = A + starts``, ``busy =
active * bin_us - idle_us`` (the load tracker's), ``u = min(busy * 8 // bin_us, 8191)`` in eighths of a
request, ``level = decodesli.bucket_of(u)``: K = 160 levels, exact below ``u = 16``, 16 per octave above.
A level's concurrency is ``lower(level) / 8``.

**Fold**, in the advance, before observing: the evicted bins ``e`` in ``(previous q_hi - B, q_hi - B]``
ascending (every ring bin from a jump of ``B`` on; none before the first step), ``A`` starting at
``carry``: a bin with ``e >= q_first`` and ``sli != 0`` adds its ``(n, b)`` to ``gen[x & 1][level(e)]``,
``x = e // epoch_bins``; then ``A += starts - ends`` and the three cells are cleared; ``carry = A`` at the
end. ``gen_epoch[2]`` is tracker-wide: for every epoch ``x`` of the evicted bins ``>= q_first``, ascending,
generation ``x & 1`` is cleared in every row when ``gen_epoch[x & 1] != x``, and ``gen_epoch[x & 1] = x``.
``epoch_bins >= B``, so one advance touches at most two epochs. ``q_first`` is the load tracker's.

**Merged curve**, from scratch every step: ``x_now = max(oldest - 1, 0) // epoch_bins``; ``long[l]`` sums
the generations whose epoch is ``x_now`` or ``x_now - 1``; ``ring[l]`` sums ``sli`` of the bins in
``[max(oldest, q_first), q_hi - settle]`` by their level; ``curve = long + ring``.

**Knee**: ``d_l = b_l * 10^6 - budget_ppm * n_l``, ``S_l`` the sum of ``d_j`` over ``j >= l``; the knee is
the largest ``l`` at which ``S_l`` attains its maximum, if that maximum is ``> 0``. It is valid when the
``n_j`` over ``j >= knee`` reach ``min_requests``. A knee that is not valid is reported as none.

**Recent**: ``(q_hi - settle - R, q_hi - settle]``, ``recent_u = min(busy_recent * 8 // (R * bin_us),
8191)``. **State**: 0 unknown (recent reaches below ``max(oldest, q_first)``, or the curve's total ``n <
min_requests``), 1 no_knee, 2 below, 3 saturated (recent level ``>=`` knee). ``age``: consecutive
saturated steps, saturating at 2^32 - 1. An unknown row keeps its totals, ``top_level`` and the curve;
its knee and recent fields are none / 0.

**Bounds**: the load tracker's ring bound, and ``curve_records_max`` (at most 2^40) over the spans offered
in the current epoch and the two before it; a step that would pass either is refused before anything
changes.

``SaturationOracle`` is these rules in numpy: the reference the device tracker (ops/csrc/satcurve.hip,
ops/satcurve.py) is tested against for equality, and what ``engine="cpu"`` uses.
"""

from __future__ import annotations

from collections import deque
from typing import Deque, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .decodesli import bucket_of, lower
from .errsli import budget_ppm  # noqa: F401 - the budget in millionths of a target
from .loadsli import (MAX_BIN_US, MAX_BINS, MAX_LATENCY_MS, MIN_BIN_US, MIN_BINS, NO_BIN, NOT_AN_END, _gather,
                      default_ring_records_max, dur_us, ordered, per_bin)
from .loadsli import ranges_of as load_ranges_of
from .onset import advance, cleared, oldest_bin
from .trackerstate import OracleCheckpoint

K = 160
MAX_U = 8191
NONE = 0xFFFFFFFF
MILLION = 1_000_000
MAX_EPOCH_BINS = (1 << 31) - 1
MAX_MIN_REQUESTS = (1 << 31) - 1
MAX_CURVE_RECORDS = 1 << 40
ROW_BYTES = 64
UNKNOWN, NO_KNEE, BELOW, SATURATED = 0, 1, 2, 3
STATE_NAMES = ("unknown", "no_knee", "below", "saturated")
# one service (ops/csrc/satcurve_host.h Row)
SAT_ROW = np.dtype([("state", "<u4"), ("knee_level", "<u4"), ("recent_u", "<u4"), ("top_level", "<u4"),
                    ("n_total", "<u8"), ("b_total", "<u8"), ("n_knee", "<u8"), ("b_knee", "<u8"), ("busy_recent", "<u8"),
                    ("age", "<u4"), ("pad", "<u4")])
assert SAT_ROW.itemsize == ROW_BYTES
# per-step statistics, in the device's order (ops/csrc/satcurve_host.h Stat)
STATS = ("observed", "out_of_group", "invalid", "no_time", "future", "too_old", "clipped", "no_ttft")
N_STATS = 8
EVENT_STATS = ("out_of_group", "invalid", "no_time", "future", "too_old", "clipped", "no_ttft")
RESULT_FIELDS = ("rows", "curve", "stats")
# what WindowPipeline.results() gains with the tracker on
RESULT_KEYS = ("sat_rows", "sat_curve", "sat_stats")


def stats_dict(stats: np.ndarray) -> Dict[str, int]:
    return {name: int(stats[i]) for i, name in enumerate(STATS)}


def result_keys(result: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """A step's results under the names WindowPipeline.results() carries (RESULT_KEYS)."""
    return {"sat_rows": np.asarray(result["rows"]), "sat_curve": np.asarray(result["curve"]),
            "sat_stats": np.asarray(result["stats"])}


def unknown_rows(n: int) -> np.ndarray:
    rows = np.zeros(int(n), SAT_ROW)
    rows["knee_level"] = NONE
    rows["top_level"] = NONE
    return rows


def empty_result(n_groups: int) -> Dict[str, np.ndarray]:
    """A window the tracker did not step for: unknown rows over an empty curve, no statistics."""
    return {"rows": unknown_rows(n_groups), "curve": np.zeros((int(n_groups), K, 2), np.uint64),
            "stats": np.zeros(N_STATS, np.uint32)}


def u_of(busy_us, span_us: int) -> np.ndarray:
    """Busy time over ``span_us`` in eighths of a request, clamped to MAX_U (int64, ``busy_us``'s shape)."""
    return np.minimum(np.maximum(np.asarray(busy_us, np.int64), 0) * 8 // int(span_us), MAX_U)


def level_of_u(u) -> np.ndarray:
    return bucket_of(u)


def concurrency_of(level: int) -> float:
    """A level's concurrency: the smallest of its eighths."""
    return float(lower(int(level))) / 8.0


def layout(group_cap: int) -> Dict[str, int]:
    """ops/csrc/satcurve_host.h layout(), in uint32 words."""
    curve = int(group_cap) * (ROW_BYTES // 4)
    stats = curve + int(group_cap) * K * 4
    return {"rows": 0, "curve": curve, "stats": stats, "words": (stats + N_STATS + 3) & ~3}


def device_bytes(bins: int, span_cap: int, group_cap: int) -> int:
    """ops/csrc/satcurve_host.h device_bytes()."""
    return int(span_cap) * 64 + int(group_cap) * int(bins) * 24 + int(group_cap) * 8 + int(group_cap) * 2 * K * 16 + \
        layout(group_cap)["words"] * 4


def check_config(bins: int, bin_us: int, settle_bins: int, recent_bins: int, epoch_bins: int, budget_ppm: int,
                 min_requests: int, slo_ms: float, span_cap: int, group_cap: int, n_buffers: int, ring_records_max: int,
                 curve_records_max: int) -> None:
    """The configuration checks of ops/csrc/satcurve_host.h validate()."""
    if not MIN_BINS <= bins <= MAX_BINS or bins & (bins - 1):
        raise ValueError("saturation curve: bins must be a power of two in [64, 8192]")
    if not MIN_BIN_US <= bin_us <= MAX_BIN_US:
        raise ValueError("saturation curve: bin_us must be in [1000, 60000000]")
    if settle_bins < 0:
        raise ValueError("saturation curve: settle_bins must be >= 0")
    if recent_bins < 1:
        raise ValueError("saturation curve: recent_bins must be >= 1")
    if settle_bins + recent_bins > bins:
        raise ValueError("saturation curve: settle_bins + recent_bins must fit the ring's bins")
    if not bins <= epoch_bins <= MAX_EPOCH_BINS:
        raise ValueError("saturation curve: epoch_bins must be in [bins, 2^31 - 1]")
    if not 1 <= budget_ppm <= MILLION - 1:
        raise ValueError("saturation curve: budget_ppm must be in [1, 999999]")
    if not 1 <= min_requests <= MAX_MIN_REQUESTS:
        raise ValueError("saturation curve: min_requests must be in [1, 2^31 - 1]")
    if not (np.isfinite(slo_ms) and slo_ms >= 0.0):
        raise ValueError("saturation curve: slo_ms must be finite and >= 0")
    if not 1 <= group_cap <= 65536:
        raise ValueError("saturation curve: group_cap must be in [1, 65536]")
    if span_cap < 1:
        raise ValueError("saturation curve: span_cap must be >= 1")
    if not 1 <= n_buffers <= 64:
        raise ValueError("saturation curve: n_buffers out of range")
    if device_bytes(bins, span_cap, group_cap) > 1 << 31:
        raise ValueError("saturation curve: the ring needs more than 2 GiB")
    if layout(group_cap)["words"] * 4 > 1 << 31:
        raise ValueError("saturation curve: a result block needs more than 2 GiB")
    if not 1 <= ring_records_max <= default_ring_records_max(bins, bin_us):
        raise ValueError("saturation curve: ring_records_max * bins * bin_us must be in [1, 2^53], "
                         "ring_records_max <= 2^31 - 1")
    if not 1 <= curve_records_max <= MAX_CURVE_RECORDS:
        raise ValueError("saturation curve: curve_records_max must be in [1, 2^40]")


def fold_of(prev: int, q_hi: int, q_first: int, bins: int) -> Tuple[int, int, int, int]:
    """ops/csrc/satcurve_host.h fold_of(): (first, count, lo, hi) of the bins an advance evicts and of
    those it folds (``lo > hi``: none)."""
    if prev == NO_BIN or q_hi <= prev:
        return 0, 0, 0, -1
    count = cleared(prev, q_hi, bins)
    first = oldest_bin(prev, bins)
    return first, count, max(first, int(q_first)), first + count - 1


def epoch_now(oldest: int, epoch_bins: int) -> int:
    return max(int(oldest) - 1, 0) // int(epoch_bins)


def gen_live(gen_epoch: int, x_now: int) -> bool:
    return gen_epoch >= 0 and gen_epoch in (x_now, x_now - 1)


def score(n: int, b: int, budget_ppm: int) -> int:
    return int(b) * MILLION - int(budget_ppm) * int(n)


def knee_of(curve: np.ndarray, budget_ppm: int, min_requests: int) -> Tuple[int, int, int, bool]:
    """(level or NONE, n, b, valid) of a curve [K, 2] in Python's unbounded integers: the largest level at
    which the suffix sum of the scores attains its maximum, if that maximum is > 0."""
    s = best = n = b = 0
    level, kn, kb = NONE, 0, 0
    for l in range(K - 1, -1, -1):
        s += score(curve[l][0], curve[l][1], budget_ppm)
        n += int(curve[l][0])
        b += int(curve[l][1])
        if s > best:
            best, level, kn, kb = s, l, n, b
    return level, kn, kb, level != NONE and kn >= int(min_requests)


def state_of(recent_known: bool, n_total: int, min_requests: int, knee_valid: bool, recent_level: int,
             knee_level: int) -> int:
    if not recent_known or int(n_total) < int(min_requests):
        return UNKNOWN
    if not knee_valid:
        return NO_KNEE
    return BELOW if int(recent_level) < int(knee_level) else SATURATED


def age_of(state: int, prev_age: int) -> int:
    return min(int(prev_age) + 1, (1 << 32) - 1) if state == SATURATED else 0


def summary(row, curve: np.ndarray) -> Dict[str, object]:
    """One SAT_ROW and its curve [K, 2] as the decision log's ``saturation`` entry; ``None`` where a value's
    denominator or its source is none."""
    state = int(row["state"])
    knee = int(row["knee_level"])
    knee_c = None if knee == NONE else concurrency_of(knee)
    recent_c = None if state == UNKNOWN else int(row["recent_u"]) / 8.0
    return {"state": STATE_NAMES[state], "age_windows": int(row["age"]), "knee_concurrency": knee_c,
            "recent_concurrency": recent_c,
            "headroom": None if knee_c is None or not recent_c else round(knee_c / recent_c, 6),
            "requests": int(row["n_total"]), "breaches": int(row["b_total"]),
            "at_knee": {"requests": None if knee == NONE else int(row["n_knee"]),
                        "breaches": None if knee == NONE else int(row["b_knee"])},
            "curve": [{"concurrency": concurrency_of(l), "requests": int(curve[l][0]), "breaches": int(curve[l][1])}
                      for l in np.nonzero(np.asarray(curve)[:, 0])[0].tolist()]}


class SaturationOracle(OracleCheckpoint):
    """The tracker's rules in numpy (see the module docstring), with the device handle's interface."""

    # checkpoint (pipeline/trackerstate.py): the fields ops/csrc/satcurve_host.h fingerprint() covers, and what is
    # kept between steps
    KIND = "saturation curve"
    FINGERPRINT = ("group_cap", "bins", "bin_us", ("settle_bins", "settle"), ("recent_bins", "recent"), "epoch_bins",
                   "budget_ppm", "min_requests", ("slo_ms", "slo"), "ring_records_max", "curve_records_max")
    STATE = ("counts", "idle", "sli", "carry", "gen", "gen_epoch", "age", "q_hi", "q_first", "held", "epochs", "n")

    def __init__(self, bins: int = 1024, bin_us: int = 500_000, settle_bins: int = 30, recent_bins: int = 30,
                 epoch_bins: int = 43200, budget_ppm: int = 10000, min_requests: int = 200, slo_ms: float = 800.0,
                 span_cap: int = 16384, group_cap: int = 64, n_buffers: int = 3, ring_records_max: Optional[int] = None,
                 curve_records_max: Optional[int] = None, device: int = 0, lds: bool = True):
        bins, bin_us = int(bins), int(bin_us)
        if ring_records_max is None:
            ring_records_max = default_ring_records_max(max(bins, 1), max(bin_us, 1))
        if curve_records_max is None:
            curve_records_max = MAX_CURVE_RECORDS
        check_config(bins, bin_us, int(settle_bins), int(recent_bins), int(epoch_bins), int(budget_ppm), int(min_requests),
                     float(slo_ms), int(span_cap), int(group_cap), int(n_buffers), int(ring_records_max),
                     int(curve_records_max))
        self.bins, self.bin_us = bins, bin_us
        self.settle, self.recent, self.epoch_bins = int(settle_bins), int(recent_bins), int(epoch_bins)
        self.budget_ppm, self.min_requests, self.slo = int(budget_ppm), int(min_requests), np.float32(slo_ms)
        self.span_cap, self.group_cap, self.nb = int(span_cap), int(group_cap), int(n_buffers)
        self.ring_records_max, self.curve_records_max = int(ring_records_max), int(curve_records_max)
        C = self.group_cap
        self.counts = np.zeros((C, bins), np.uint64)  # slot order
        self.idle = np.zeros((C, bins), np.uint64)
        self.sli = np.zeros((C, bins), np.uint64)
        self.carry = np.zeros(C, np.int32)
        self.gen = np.zeros((2, C, K, 2), np.uint64)
        self.gen_epoch = [-1, -1]
        self.age = np.zeros(C, np.uint32)
        self.q_hi = self.q_first = NO_BIN
        self.held: Deque[Tuple[int, int]] = deque()    # (q_hi of the step, spans offered)
        self.epochs: Deque[List[int]] = deque()        # [epoch of the step's q_hi, spans offered]
        self.res: Dict[int, Tuple[int, dict]] = {}
        self.n = 0

    # ---- one window ---------------------------------------------------------------------------
    def step(self, span_ranges: Sequence[Tuple[int, int]], cut_ns: int, n_groups: int) -> int:
        """``span_ranges`` = [(host address, bytes)] of 64-byte SPAN records, as the engine gets them."""
        for a, nbytes in span_ranges:
            if int(nbytes) and not int(a):
                raise ValueError("saturation curve step: null range")
            if int(nbytes) % 64:
                raise ValueError("saturation curve step: a range is not whole 64-byte spans")
        return self.step_records(_gather(span_ranges), cut_ns, n_groups)

    def ring_after(self, q_hi: int, n: int) -> int:
        return int(n) + sum(c for q, c in self.held if q > q_hi - self.bins)

    def curve_after(self, q_hi: int, n: int) -> int:
        x = int(q_hi) // self.epoch_bins
        return int(n) + sum(c for e, c in self.epochs if e >= x - 2)

    def step_records(self, spans: np.ndarray, cut_ns: int, n_groups: int) -> int:
        G, C, B, bin_us = int(n_groups), self.group_cap, self.bins, self.bin_us
        if int(cut_ns) <= 0:
            raise ValueError("saturation curve step: cut_ns must be > 0")
        if not 0 <= G <= C:
            raise ValueError("saturation curve step: n_groups out of range")
        if len(spans) > self.span_cap:
            raise ValueError("saturation curve step: more spans than span_cap")
        prev, q_hi = self.q_hi, advance(self.q_hi, int(cut_ns) // 1000, bin_us)
        if self.ring_after(q_hi, len(spans)) > self.ring_records_max:
            raise ValueError("saturation curve step: the ring would hold more than ring_records_max spans")
        if self.curve_after(q_hi, len(spans)) > self.curve_records_max:
            raise ValueError("saturation curve step: the curve would hold more than curve_records_max spans")
        # nothing has changed up to here
        while self.held and self.held[0][0] <= q_hi - B:
            self.held.popleft()
        x_hi = q_hi // self.epoch_bins
        while self.epochs and self.epochs[0][0] < x_hi - 2:
            self.epochs.popleft()
        if len(spans):
            self.held.append((q_hi, len(spans)))
            if self.epochs and self.epochs[-1][0] == x_hi:
                self.epochs[-1][1] += len(spans)
            else:
                self.epochs.append([x_hi, len(spans)])
        self._fold(prev, q_hi)
        self.q_hi = q_hi
        if prev == NO_BIN or q_hi - prev >= B:
            self.q_first = q_hi
        oldest = oldest_bin(q_hi, B)

        flags = spans["flags"].astype(np.uint32)
        grp = spans["group_id"].astype(np.int64)
        v = np.ascontiguousarray(spans["latency_ms"], dtype=np.float32)
        ends_request = (flags & np.uint32(NOT_AN_END)) == 0
        in_group = ends_request & (grp < G)
        with np.errstate(invalid="ignore"):
            valid = in_group & (v >= np.float32(0.0)) & (v <= np.float32(MAX_LATENCY_MS))
        timed = valid & (spans["ts_ns"].astype(np.int64) > 0)
        at = np.nonzero(timed)[0]
        g = grp[at]
        ts = spans["ts_ns"][at].astype(np.int64) // 1000
        ttft = np.ascontiguousarray(spans["ttft_ms"], dtype=np.float32)[at]
        with np.errstate(invalid="ignore"):
            has = ttft >= np.float32(0.0)
            add = np.uint64(1) + ((ttft > self.slo).astype(np.uint64) << np.uint64(32))
        te = ts + dur_us(v[at])
        qs, qe = ts // bin_us, te // bin_us
        ahead = qs > q_hi
        cut = ~ahead & (qe > q_hi)
        ts = np.where(ahead, q_hi * bin_us, ts)
        te = np.where(ahead, q_hi * bin_us, np.where(cut, (q_hi + 1) * bin_us, te))
        qs = np.where(ahead, q_hi, qs)
        qe = np.where(ahead | cut, q_hi, qe)
        too_old = qe < oldest
        clipped = ~too_old & (qs < oldest)
        start = ~too_old & ~clipped
        end = ~too_old
        np.add.at(self.carry, g[clipped], np.int32(1))
        np.add.at(self.counts, (g[start], qs[start] & (B - 1)), np.uint64(1))
        np.add.at(self.idle, (g[start], qs[start] & (B - 1)), (ts - qs * bin_us)[start].astype(np.uint64))
        np.add.at(self.sli, (g[start & has], qs[start & has] & (B - 1)), add[start & has])
        np.add.at(self.counts, (g[end], qe[end] & (B - 1)), np.uint64(1 << 32))
        np.add.at(self.idle, (g[end], qe[end] & (B - 1)), ((qe + 1) * bin_us - te)[end].astype(np.uint64))
        stats = np.zeros(N_STATS, np.uint32)
        stats[:] = [len(at), int((ends_request & (grp >= G)).sum()), int((in_group & ~valid).sum()),
                    int((valid & ~timed).sum()), int((ahead | cut).sum()), int(too_old.sum()), int(clipped.sum()),
                    int((~has).sum())]

        rows, curve = self._rows()
        idx = self.n
        self.res[idx % self.nb] = (idx, {"rows": rows, "curve": curve, "stats": stats})
        self.n += 1
        return idx

    def _fold(self, prev: int, q_hi: int) -> None:
        """The advance: the evicted bins into their generations, their cells cleared, carry moved on."""
        B, bin_us = self.bins, self.bin_us
        first, count, lo, hi = fold_of(prev, q_hi, self.q_first, B)
        if not count:
            return
        if lo <= hi:
            for x in range(lo // self.epoch_bins, hi // self.epoch_bins + 1):
                if self.gen_epoch[x & 1] != x:
                    self.gen[x & 1] = 0
                    self.gen_epoch[x & 1] = x
        e = first + np.arange(count, dtype=np.int64)
        slots = e & (B - 1)
        ev = self.counts[:, slots]
        starts = (ev & np.uint64(0xFFFFFFFF)).astype(np.int64)
        delta = starts - (ev >> np.uint64(32)).astype(np.int64)
        after = self.carry.astype(np.int64)[:, None] + np.cumsum(delta, axis=1)
        busy = (after - delta + starts) * bin_us - self.idle[:, slots].astype(np.int64)
        level = level_of_u(u_of(busy, bin_us))
        x = self.sli[:, slots]
        row, col = np.nonzero((x != 0) & (e >= lo)[None, :])
        par = (e[col] // self.epoch_bins) & 1 if len(col) else col
        np.add.at(self.gen, (par, row, level[row, col], 0), x[row, col] & np.uint64(0xFFFFFFFF))
        np.add.at(self.gen, (par, row, level[row, col], 1), x[row, col] >> np.uint64(32))
        self.carry[:] = after[:, -1].astype(np.int32)
        self.counts[:, slots] = 0
        self.idle[:, slots] = 0
        self.sli[:, slots] = 0

    def _rows(self) -> Tuple[np.ndarray, np.ndarray]:
        """Every row of group_cap and its merged curve from the ring and the generations; updates ``age``."""
        C, B, q_hi, bin_us = self.group_cap, self.bins, self.q_hi, self.bin_us
        _, _, _, busy = per_bin(self.counts, self.idle, self.carry, q_hi, bin_us)
        r = load_ranges_of(q_hi, self.q_first, B, self.settle, self.recent, 1)
        q0, lo, settled_hi = r["oldest"], r["lo"], r["recent_hi"]
        recent_known = r["recent_lo"] >= lo
        curve = np.zeros((C, K, 2), np.uint64)
        x_now = epoch_now(q0, self.epoch_bins)
        for p in (0, 1):
            if gen_live(self.gen_epoch[p], x_now):
                curve += self.gen[p]
        if settled_hi >= lo:
            cols = slice(lo - q0, settled_hi - q0 + 1)
            x = ordered(self.sli, q_hi)[:, cols]
            level = level_of_u(u_of(busy[:, cols], bin_us))
            row, col = np.nonzero(x != 0)
            np.add.at(curve, (row, level[row, col], 0), x[row, col] & np.uint64(0xFFFFFFFF))
            np.add.at(curve, (row, level[row, col], 1), x[row, col] >> np.uint64(32))
        busy_recent = busy[:, r["recent_lo"] - q0:r["recent_hi"] - q0 + 1].sum(axis=1) if recent_known else np.zeros(C, np.int64)
        rows = unknown_rows(C)
        for g in range(C):
            n_total, b_total = int(curve[g, :, 0].sum()), int(curve[g, :, 1].sum())
            assert n_total <= self.curve_records_max, "saturation curve: more requests than curve_records_max"
            rows["n_total"][g], rows["b_total"][g] = n_total, b_total
            have = np.nonzero(curve[g, :, 0])[0]
            if len(have):
                rows["top_level"][g] = have[-1]
            level, kn, kb, valid = knee_of(curve[g].tolist(), self.budget_ppm, self.min_requests)
            recent_u = int(u_of(busy_recent[g], self.recent * bin_us))
            state = state_of(recent_known, n_total, self.min_requests, valid, int(level_of_u(recent_u)), level)
            rows["state"][g] = state
            if state != UNKNOWN:
                rows["recent_u"][g], rows["busy_recent"][g] = recent_u, busy_recent[g]
                if valid:
                    rows["knee_level"][g], rows["n_knee"][g], rows["b_knee"][g] = level, kn, kb
            rows["age"][g] = age_of(state, int(self.age[g]))
        self.age[:] = rows["age"]
        return rows, curve

    # ---- results ------------------------------------------------------------------------------
    def query(self, i: int) -> bool:
        return True

    def _held(self, i: int):
        held = self.res.get(int(i) % self.nb)
        if held is None or held[0] != int(i):
            raise IndexError(f"saturation curve step {i} is not held (only the last {self.nb})")
        return held

    def results(self, i: int, n_groups: int) -> Dict[str, np.ndarray]:
        held = self._held(i)
        G = int(n_groups)
        if not 0 <= G <= self.group_cap:
            raise ValueError("n_groups")
        return {"rows": held[1]["rows"][:G].copy(), "curve": held[1]["curve"][:G].copy(), "stats": held[1]["stats"].copy()}

    def block(self, i: int) -> np.ndarray:
        """Step ``i``'s whole result block as the device lays it out, uint32 words."""
        held = self._held(i)[1]
        lay = layout(self.group_cap)
        out = np.zeros(lay["words"], np.uint32)
        out[lay["rows"]:lay["curve"]] = np.ascontiguousarray(held["rows"]).view(np.uint32).ravel()
        out[lay["curve"]:lay["stats"]] = np.ascontiguousarray(held["curve"]).view(np.uint32).ravel()
        out[lay["stats"]:lay["stats"] + N_STATS] = held["stats"]
        return out

    def step_ms(self, i: int) -> Tuple[float, float]:
        return 0.0, 0.0

    def observe_ms(self, i: int) -> float:
        return 0.0

    def resident(self) -> Dict[str, object]:
        """Everything kept between steps: ``counts`` / ``idle_us`` / ``sli`` [group_cap, B] in slot order,
        ``carry``, ``gen`` [2, group_cap, K, 2], ``gen_epoch``, ``age``, ``q_hi``, ``q_first``."""
        return {"counts": self.counts.copy(), "idle_us": self.idle.copy(), "sli": self.sli.copy(),
                "carry": self.carry.copy(), "gen": self.gen.copy(), "gen_epoch": tuple(int(x) for x in self.gen_epoch),
                "age": self.age.copy(), "q_hi": int(self.q_hi), "q_first": int(self.q_first)}

    def sync(self) -> None:
        pass

    def close(self) -> None:
        pass
