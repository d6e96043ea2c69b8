"""Load SLI per service on the host: the rules of the load tracker (traffic and saturation).

Every other tracker looks at latency or at errors. This one answers whether load went up: per service,
over a ring of absolute time bins, the arrivals, the completions, the requests in flight and the exact
in-flight (busy) time, from the start ``ts_ns`` and the duration ``latency_ms`` that every record
ending a request carries. By Little's law ``L = lambda * W``: when the concurrency of the recent bins
grew with the arrivals the service is in a **surge**, when it grew at the same arrivals it is in a
**slowdown**. Everything is in integers: device and oracle are compared for equality.

**Which records count**: 64-byte SPAN records, in this order: SPAN_START or SPAN_FIRST_TOKEN: skipped
(they do not end a request; no other flag bit and not ``ttft_ms`` matter); ``group_id >= n_groups``:
``out_of_group``; ``latency_ms`` NaN, ``< 0`` or ``> 86_400_000`` in a float32 compare: ``invalid``;
``ts_ns <= 0``: ``no_time``; else ``observed``.

**Times** in microseconds: ``ts_us = ts_ns // 1000``, ``dur_us = int64(trunc(float64(latency_ms) *
1000.0))`` (one IEEE double multiply), ``te_us = ts_us + dur_us``; the request occupies ``[ts_us,
te_us)``, ``qs = ts_us // bin_us``, ``qe = te_us // bin_us``. ``dur_us > settle_bins * bin_us``: also
``long``.

**Ring**: ``B`` bins per service (a power of two), slot ``q & (B - 1)``; ``q_hi = max(previous q_hi,
(cut_ns // 1000) // bin_us)`` (-1 before the first step), ``oldest = q_hi - B + 1``. Per (service,
slot) two u64 cells: ``counts`` (starts in the low word, ends in the high one) and ``idle_us``; per
service ``carry`` (int32): the requests in flight at the end of bin ``oldest - 1``.

**Advance**, before observing: for every bin in ``(previous q_hi, q_hi]`` the evicted bin is folded,
``carry += starts - ends``, and its slot cleared, in every row; a jump of ``B`` or more folds and
clears everything. ``q_first`` is ``q_hi`` after the first step and again after such a jump.

**Placement** of an observed record: ``qs > q_hi``: ``future``, a zero-length request in ``q_hi``
(``starts += 1``, ``ends += 1``, ``idle_us += bin_us``). Else ``qe > q_hi``: ``future``, ``te_us :=
(q_hi + 1) * bin_us``, ``qe := q_hi``, and on. ``qe < oldest``: ``too_old``, placed nowhere. ``qs <
oldest <= qe``: ``clipped``, ``carry += 1``, only the end placed. Otherwise at ``qs``: ``starts += 1``,
``idle_us += ts_us - qs * bin_us``. In every placed case at ``qe``: ``ends += 1``, ``idle_us += (qe + 1)
* bin_us - te_us``.

**Per bin** from ``oldest`` to ``q_hi``, ``A`` starting at ``carry``: ``active = A + starts`` (requests
touching the bin), ``busy = active * bin_us - idle_us`` (their exact time inside it), ``A += starts -
ends``. ``A >= 0`` after every bin and ``A == 0`` after ``q_hi`` (every observed request has finished):
the oracle asserts both.

**Ranges**: ``recent = (q_hi - settle - R, q_hi - settle]``, ``base = [max(oldest, q_first), q_hi -
settle - R]``, ``base_bins`` its length clamped at 0. The row is **warming** while ``recent`` reaches
below ``max(oldest, q_first)`` or ``base_bins < min_base_bins``. The newest ``settle`` bins are left
out: a request still in flight is invisible until it finishes.

**Classification** with ``nb = base_bins``, ``nr = R``, ``conc_X_milli = busy_X * 1000 // (bins_X *
bin_us)``: ``arr_up``: ``arr_recent >= min_requests`` and ``arr_recent * nb * 1000 >= f * arr_base *
nr``; ``arr_down``: ``arr_base * nr >= min_requests * nb`` and ``arr_recent * nb * f <= 1000 * arr_base *
nr``; ``conc_up``: ``conc_recent_milli >= min_conc_milli`` and ``conc_recent_milli * 1000 >= f *
conc_base_milli``. ``flags`` bits 0, 1, 2 = arr_up, conc_up, arr_down. ``state``: 4 warming, else 1
surge (arr_up), else 2 slowdown (conc_up), else 3 drop (arr_down), else 0 steady. ``age``: consecutive
steps in the same state among 1..3, saturating at 2^32 - 1; 0 otherwise.

**Row** (``LOAD_ROW``, 80 bytes: the fields take 72, padded to whole 16-byte stores). A warming row
carries the ring totals and the peak; its range fields (``base_bins`` and ``flags`` too) are 0.

**The bound**: ``ring_records_max * B * bin_us <= 2^53`` (default: the largest such value, capped at
2^31 - 1); the tracker keeps (``q_hi`` of the step, spans offered) and refuses a step that would pass
it before anything changes. Then every busy sum stays below 2^53 and every product above in 64 bits.

``LoadSliOracle`` is these rules in numpy: the reference the device tracker (ops/csrc/loadsli.hip,
ops/loadsli.py) is tested against for equality, and what ``engine="cpu"`` uses.
"""

from __future__ import annotations

from collections import deque
from typing import Deque, Dict, Optional, Sequence, Tuple

import numpy as np

from ..collector import records
from .trackerstate import OracleCheckpoint
from .onset import advance, cleared, oldest_bin

MIN_BINS, MAX_BINS = 64, 8192
MIN_BIN_US, MAX_BIN_US = 1000, 60_000_000
MAX_LATENCY_MS = 86_400_000
MAX_RING_RECORDS = (1 << 31) - 1
MAX_PRODUCT = 1 << 53
MIN_FACTOR_MILLI, MAX_FACTOR_MILLI = 1001, 64000
MAX_MIN_REQUESTS = (1 << 31) - 1
MAX_MIN_CONC_MILLI = 1_000_000_000
ROW_BYTES = 80
NO_BIN = -1
STEADY, SURGE, SLOWDOWN, DROP, WARMING = 0, 1, 2, 3, 4
STATE_NAMES = ("steady", "surge", "slowdown", "drop", "warming")
ARR_UP, CONC_UP, ARR_DOWN = 1, 2, 4
NOT_AN_END = records.SPAN_FIRST_TOKEN | records.SPAN_START
# one service (ops/csrc/loadsli_host.h Row)
LOAD_ROW = np.dtype([("state", "<u4"), ("age", "<u4"), ("peak_q", "<i8"), ("busy_recent", "<u8"), ("busy_base", "<u8"),
                     ("busy_ring", "<u8"), ("arr_recent", "<u4"), ("arr_base", "<u4"), ("done_recent", "<u4"),
                     ("done_base", "<u4"), ("peak_active", "<u4"), ("base_bins", "<u4"), ("arr_ring", "<u4"),
                     ("flags", "<u4"), ("pad", "<u4", (2,))])
assert LOAD_ROW.itemsize == ROW_BYTES
# per-step statistics, in the device's order (ops/csrc/loadsli_host.h Stat)
STATS = ("observed", "out_of_group", "invalid", "no_time", "future", "too_old", "clipped", "long")
N_STATS = 8
EVENT_STATS = ("out_of_group", "invalid", "no_time", "future", "too_old", "clipped", "long")
RESULT_FIELDS = ("rows", "stats")
# what WindowPipeline.results() gains with the tracker on
RESULT_KEYS = ("load_rows", "load_stats")


def stats_dict(stats: np.ndarray) -> Dict[str, int]:
    return {name: int(stats[i]) for i, name in enumerate(STATS)}


def result_keys(result: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """A step's results under the names WindowPipeline.results() carries (RESULT_KEYS)."""
    return {"load_rows": np.asarray(result["rows"]), "load_stats": np.asarray(result["stats"])}


def warming_rows(n: int) -> np.ndarray:
    rows = np.zeros(int(n), LOAD_ROW)
    rows["state"] = WARMING
    rows["peak_q"] = NO_BIN
    return rows


def empty_result(n_groups: int) -> Dict[str, np.ndarray]:
    """A window the tracker did not step for: warming rows over an empty ring, no statistics."""
    return {"rows": warming_rows(n_groups), "stats": np.zeros(N_STATS, np.uint32)}


def dur_us(latency_ms) -> np.ndarray:
    """Valid float32 latencies in whole microseconds: one double multiply, truncated."""
    return np.trunc(np.asarray(latency_ms, np.float32).astype(np.float64) * 1000.0).astype(np.int64)


def layout(group_cap: int) -> Dict[str, int]:
    """ops/csrc/loadsli_host.h layout(), in uint32 words."""
    stats = int(group_cap) * (ROW_BYTES // 4)
    return {"rows": 0, "stats": stats, "words": (stats + N_STATS + 3) & ~3}


def device_bytes(bins: int, span_cap: int, group_cap: int) -> int:
    """ops/csrc/loadsli_host.h device_bytes()."""
    return int(span_cap) * 64 + int(group_cap) * int(bins) * 16 + int(group_cap) * 12 + layout(group_cap)["words"] * 4


def default_ring_records_max(bins: int, bin_us: int) -> int:
    return min(MAX_RING_RECORDS, MAX_PRODUCT // (int(bins) * int(bin_us)))


def check_config(bins: int, bin_us: int, settle_bins: int, recent_bins: int, min_base_bins: int, factor_milli: int,
                 min_requests: int, min_conc_milli: int, span_cap: int, group_cap: int, n_buffers: int,
                 ring_records_max: int) -> None:
    """The configuration checks of ops/csrc/loadsli_host.h validate()."""
    if not MIN_BINS <= bins <= MAX_BINS or bins & (bins - 1):
        raise ValueError("load sli: bins must be a power of two in [64, 8192]")
    if not MIN_BIN_US <= bin_us <= MAX_BIN_US:
        raise ValueError("load sli: bin_us must be in [1000, 60000000]")
    if settle_bins < 0:
        raise ValueError("load sli: settle_bins must be >= 0")
    if recent_bins < 1:
        raise ValueError("load sli: recent_bins must be >= 1")
    if min_base_bins < 1:
        raise ValueError("load sli: min_base_bins must be >= 1")
    if settle_bins + recent_bins + min_base_bins > bins:
        raise ValueError("load sli: settle_bins + recent_bins + min_base_bins must fit the ring's bins")
    if not MIN_FACTOR_MILLI <= factor_milli <= MAX_FACTOR_MILLI:
        raise ValueError("load sli: factor_milli must be in [1001, 64000]")
    if not 1 <= min_requests <= MAX_MIN_REQUESTS:
        raise ValueError("load sli: min_requests must be in [1, 2^31 - 1]")
    if not 1 <= min_conc_milli <= MAX_MIN_CONC_MILLI:
        raise ValueError("load sli: min_conc_milli must be in [1, 1000000000]")
    if not 1 <= group_cap <= 65536:
        raise ValueError("load sli: group_cap must be in [1, 65536]")
    if span_cap < 1:
        raise ValueError("load sli: span_cap must be >= 1")
    if not 1 <= n_buffers <= 64:
        raise ValueError("load sli: n_buffers out of range")
    if device_bytes(bins, span_cap, group_cap) > 1 << 31:
        raise ValueError("load sli: the ring needs more than 2 GiB")
    if not 1 <= ring_records_max <= default_ring_records_max(bins, bin_us):
        raise ValueError("load sli: ring_records_max * bins * bin_us must be in [1, 2^53], ring_records_max <= 2^31 - 1")


def _gather(ranges) -> np.ndarray:
    from .cpu import _gather as g

    b = g(ranges)
    return b.view(records.SPAN) if len(b) else np.zeros(0, records.SPAN)


def ordered(cells: np.ndarray, q_hi: int) -> np.ndarray:
    """Cells [C, B] (slot order) in ring order: column 0 = the oldest bin."""
    B = cells.shape[1]
    return cells[:, (np.arange(B, dtype=np.int64) + oldest_bin(q_hi, B)) & (B - 1)]


def ranges_of(q_hi: int, q_first: int, bins: int, settle: int, recent: int, min_base_bins: int) -> Dict[str, int]:
    """ops/csrc/loadsli_host.h ranges_of(): inclusive bin ranges."""
    oldest = oldest_bin(q_hi, bins)
    lo = max(oldest, int(q_first))
    recent_hi = int(q_hi) - int(settle)
    recent_lo = recent_hi - int(recent) + 1
    base_bins = max(0, recent_lo - lo)
    return {"oldest": oldest, "lo": lo, "recent_lo": recent_lo, "recent_hi": recent_hi, "base_lo": lo,
            "base_hi": recent_lo - 1, "base_bins": base_bins,
            "warming": bool(recent_lo < lo or base_bins < int(min_base_bins))}


def classify(busy_recent: int, busy_base: int, arr_recent: int, arr_base: int, base_bins: int, recent_bins: int,
             bin_us: int, factor_milli: int, min_requests: int, min_conc_milli: int) -> Tuple[int, int]:
    """(flags, state) of a row that is not warming, in Python's unbounded integers."""
    ar, ab, nb, nr, f = int(arr_recent), int(arr_base), int(base_bins), int(recent_bins), int(factor_milli)
    flags = 0
    if ar >= min_requests and ar * nb * 1000 >= f * ab * nr:
        flags |= ARR_UP
    if ab * nr >= min_requests * nb and ar * nb * f <= 1000 * ab * nr:
        flags |= ARR_DOWN
    cr = int(busy_recent) * 1000 // (nr * int(bin_us))
    cb = int(busy_base) * 1000 // (nb * int(bin_us))
    if cr >= min_conc_milli and cr * 1000 >= f * cb:
        flags |= CONC_UP
    state = SURGE if flags & ARR_UP else SLOWDOWN if flags & CONC_UP else DROP if flags & ARR_DOWN else STEADY
    return flags, state


def age_of(state: int, prev_state: int, prev_age: int) -> int:
    if not SURGE <= state <= DROP:
        return 0
    if state != prev_state:
        return 1
    return min(int(prev_age) + 1, (1 << 32) - 1)


def per_bin(counts: np.ndarray, idle: np.ndarray, carry: np.ndarray, q_hi: int, bin_us: int):
    """(starts, ends, active, busy) [C, B] in ring order, by the recurrence as a prefix sum; asserts
    the invariants ``A >= 0`` after every bin and ``A == 0`` after ``q_hi``."""
    c = ordered(np.asarray(counts, np.uint64), q_hi)
    starts = (c & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ends = (c >> np.uint64(32)).astype(np.int64)
    after = np.asarray(carry, np.int64)[:, None] + np.cumsum(starts - ends, axis=1)
    assert (np.asarray(carry) >= 0).all() and (after >= 0).all(), "load sli: negative requests in flight"
    assert (after[:, -1] == 0).all(), "load sli: requests in flight after q_hi"
    active = after - (starts - ends) + starts
    busy = active * int(bin_us) - ordered(np.asarray(idle, np.uint64), q_hi).astype(np.int64)
    assert (busy >= 0).all(), "load sli: negative busy time"
    return starts, ends, active, busy


def summary(row, bin_us: int, recent_bins: int) -> Dict[str, object]:
    """One LOAD_ROW as the decision log's ``load`` entry: rates per second, concurrencies as busy time
    over the range's time, service times as busy time per completion; None where the denominator is 0."""
    state, nb, nr, bin_us = int(row["state"]), int(row["base_bins"]), int(recent_bins), int(bin_us)
    warming = state == WARMING

    def per_s(n, bins_):
        return None if warming or not bins_ else round(int(n) * 1e6 / (bins_ * bin_us), 6)

    def conc(busy, bins_):
        return None if warming or not bins_ else round(int(busy) / (bins_ * bin_us), 6)

    def svc_ms(busy, done):
        return None if warming or not int(done) else round(int(busy) / int(done) / 1000.0, 6)

    peak_q = int(row["peak_q"])
    return {"state": STATE_NAMES[state], "age_windows": int(row["age"]), "warming": warming,
            "arrivals_per_s": {"recent": per_s(row["arr_recent"], nr), "base": per_s(row["arr_base"], nb)},
            "concurrency": {"recent": conc(row["busy_recent"], nr), "base": conc(row["busy_base"], nb),
                            "peak": int(row["peak_active"]), "peak_ts_ns": peak_q * bin_us * 1000 if peak_q >= 0 else None},
            "service_time_ms": {"recent": svc_ms(row["busy_recent"], row["done_recent"]),
                                "base": svc_ms(row["busy_base"], row["done_base"])}}


class LoadSliOracle(OracleCheckpoint):
    """The tracker's rules in numpy (see the module docstring), with the device handle's interface."""

    # checkpoint (pipeline/trackerstate.py): the fields ops/csrc/loadsli_host.h fingerprint() covers, and what is
    # kept between steps
    KIND = "load sli"
    FINGERPRINT = ("group_cap", "bins", "bin_us", ("settle_bins", "settle"), ("recent_bins", "recent"), "min_base_bins",
                   ("factor_milli", "f"), "min_requests", "min_conc_milli", "ring_records_max")
    STATE = ("counts", "idle", "carry", "age", "prev_state", "q_hi", "q_first", "held", "n")

    def __init__(self, bins: int = 1024, bin_us: int = 500_000, settle_bins: int = 30, recent_bins: int = 30,
                 min_base_bins: int = 60, factor_milli: int = 1500, min_requests: int = 20, min_conc_milli: int = 1000,
                 span_cap: int = 16384, group_cap: int = 64, n_buffers: int = 3, ring_records_max: Optional[int] = None,
                 device: int = 0, lds: bool = True):
        bins, bin_us = int(bins), int(bin_us)
        if ring_records_max is None:
            ring_records_max = default_ring_records_max(max(bins, 1), max(bin_us, 1))
        check_config(bins, bin_us, int(settle_bins), int(recent_bins), int(min_base_bins), int(factor_milli),
                     int(min_requests), int(min_conc_milli), int(span_cap), int(group_cap), int(n_buffers),
                     int(ring_records_max))
        self.bins, self.bin_us = bins, bin_us
        self.settle, self.recent, self.min_base_bins = int(settle_bins), int(recent_bins), int(min_base_bins)
        self.f, self.min_requests, self.min_conc_milli = int(factor_milli), int(min_requests), int(min_conc_milli)
        self.span_cap, self.group_cap, self.nb = int(span_cap), int(group_cap), int(n_buffers)
        self.ring_records_max = int(ring_records_max)
        self.counts = np.zeros((self.group_cap, bins), np.uint64)  # slot order
        self.idle = np.zeros((self.group_cap, bins), np.uint64)
        self.carry = np.zeros(self.group_cap, np.int32)
        self.age = np.zeros(self.group_cap, np.uint32)
        self.prev_state = np.zeros(self.group_cap, np.uint32)
        self.q_hi = self.q_first = NO_BIN
        self.held: Deque[Tuple[int, int]] = deque()  # (q_hi of the step, spans offered)
        self.res: Dict[int, Tuple[int, dict]] = {}
        self.n = 0

    # ---- one window ---------------------------------------------------------------------------
    def step(self, span_ranges: Sequence[Tuple[int, int]], cut_ns: int, n_groups: int) -> int:
        """``span_ranges`` = [(host address, bytes)] of 64-byte SPAN records, as the engine gets them."""
        for a, nbytes in span_ranges:
            if int(nbytes) and not int(a):
                raise ValueError("load sli step: null range")
            if int(nbytes) % 64:
                raise ValueError("load sli step: a range is not whole 64-byte spans")
        return self.step_records(_gather(span_ranges), cut_ns, n_groups)

    def population_after(self, q_hi: int, n: int) -> int:
        return int(n) + sum(c for q, c in self.held if q > q_hi - self.bins)

    def step_records(self, spans: np.ndarray, cut_ns: int, n_groups: int) -> int:
        G, C, B, bin_us = int(n_groups), self.group_cap, self.bins, self.bin_us
        if int(cut_ns) <= 0:
            raise ValueError("load sli step: cut_ns must be > 0")
        if not 0 <= G <= C:
            raise ValueError("load sli step: n_groups out of range")
        if len(spans) > self.span_cap:
            raise ValueError("load sli step: more spans than span_cap")
        prev, q_hi = self.q_hi, advance(self.q_hi, int(cut_ns) // 1000, bin_us)
        if self.population_after(q_hi, len(spans)) > self.ring_records_max:
            raise ValueError("load sli step: the ring would hold more than ring_records_max spans")
        # nothing has changed up to here
        while self.held and self.held[0][0] <= q_hi - B:
            self.held.popleft()
        if len(spans):
            self.held.append((q_hi, len(spans)))
        self.q_hi = q_hi
        if prev == NO_BIN or q_hi - prev >= B:
            self.q_first = q_hi
        if q_hi > prev:  # the evicted bins sit in the slots of the bins that enter
            slots = (prev + 1 + np.arange(cleared(prev, q_hi, B), dtype=np.int64)) & (B - 1)
            ev = self.counts[:, slots]
            self.carry += ((ev & np.uint64(0xFFFFFFFF)).astype(np.int64) - (ev >> np.uint64(32)).astype(np.int64)) \
                .sum(axis=1).astype(np.int32)
            self.counts[:, slots] = 0
            self.idle[:, slots] = 0
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
        dur = dur_us(v[at])
        te = ts + dur
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
        np.add.at(self.counts, (g[end], qe[end] & (B - 1)), np.uint64(1 << 32))
        np.add.at(self.idle, (g[end], qe[end] & (B - 1)), ((qe + 1) * bin_us - te)[end].astype(np.uint64))
        stats = np.zeros(N_STATS, np.uint32)
        stats[:] = [len(at), int((ends_request & (grp >= G)).sum()), int((in_group & ~valid).sum()),
                    int((valid & ~timed).sum()), int((ahead | cut).sum()), int(too_old.sum()), int(clipped.sum()),
                    int((dur > self.settle * bin_us).sum())]

        rows = self._rows()
        idx = self.n
        self.res[idx % self.nb] = (idx, {"rows": rows, "stats": stats})
        self.n += 1
        return idx

    def _rows(self) -> np.ndarray:
        """Every row of group_cap from the ring; updates ``age`` and the previous state."""
        C, B, q_hi = self.group_cap, self.bins, self.q_hi
        starts, ends, active, busy = per_bin(self.counts, self.idle, self.carry, q_hi, self.bin_us)
        r = ranges_of(q_hi, self.q_first, B, self.settle, self.recent, self.min_base_bins)
        q0 = r["oldest"]
        rows = warming_rows(C)
        rows["busy_ring"] = busy.sum(axis=1).astype(np.uint64)
        rows["arr_ring"] = starts.sum(axis=1).astype(np.uint32)
        peak = active.max(axis=1)
        rows["peak_active"] = peak.astype(np.uint32)
        rows["peak_q"] = np.where(peak > 0, q0 + active.argmax(axis=1), NO_BIN)  # argmax: the first maximum
        if not r["warming"]:
            rec = slice(r["recent_lo"] - q0, r["recent_hi"] - q0 + 1)
            base = slice(r["base_lo"] - q0, r["base_hi"] - q0 + 1)
            rows["busy_recent"], rows["busy_base"] = busy[:, rec].sum(axis=1), busy[:, base].sum(axis=1)
            rows["arr_recent"], rows["arr_base"] = starts[:, rec].sum(axis=1), starts[:, base].sum(axis=1)
            rows["done_recent"], rows["done_base"] = ends[:, rec].sum(axis=1), ends[:, base].sum(axis=1)
            rows["base_bins"] = r["base_bins"]
            for g in range(C):
                rows["flags"][g], rows["state"][g] = classify(
                    rows["busy_recent"][g], rows["busy_base"][g], rows["arr_recent"][g], rows["arr_base"][g],
                    r["base_bins"], self.recent, self.bin_us, self.f, self.min_requests, self.min_conc_milli)
        for g in range(C):
            rows["age"][g] = age_of(int(rows["state"][g]), int(self.prev_state[g]), int(self.age[g]))
        self.age[:] = rows["age"]
        self.prev_state[:] = rows["state"]
        return rows

    # ---- results ------------------------------------------------------------------------------
    def query(self, i: int) -> bool:
        return True

    def _held(self, i: int):
        held = self.res.get(int(i) % self.nb)
        if held is None or held[0] != int(i):
            raise IndexError(f"load sli step {i} is not held (only the last {self.nb})")
        return held

    def results(self, i: int, n_groups: int) -> Dict[str, np.ndarray]:
        held = self._held(i)
        G = int(n_groups)
        if not 0 <= G <= self.group_cap:
            raise ValueError("n_groups")
        return {"rows": held[1]["rows"][:G].copy(), "stats": held[1]["stats"].copy()}

    def block(self, i: int) -> np.ndarray:
        """Step ``i``'s whole result block as the device lays it out, uint32 words."""
        held = self._held(i)[1]
        lay = layout(self.group_cap)
        out = np.zeros(lay["words"], np.uint32)
        out[lay["rows"]:lay["stats"]] = np.ascontiguousarray(held["rows"]).view(np.uint32).ravel()
        out[lay["stats"]:lay["stats"] + N_STATS] = held["stats"]
        return out

    def step_ms(self, i: int) -> Tuple[float, float]:
        return 0.0, 0.0

    def observe_ms(self, i: int) -> float:
        return 0.0

    def resident(self) -> Dict[str, np.ndarray]:
        """Everything kept between steps: ``counts`` / ``idle_us`` [group_cap, B] in slot order,
        ``carry``, ``age``, ``prev_state``, ``q_hi``, ``q_first``."""
        return {"counts": self.counts.copy(), "idle_us": self.idle.copy(), "carry": self.carry.copy(),
                "age": self.age.copy(), "prev_state": self.prev_state.copy(), "q_hi": int(self.q_hi),
                "q_first": int(self.q_first)}

    def sync(self) -> None:
        pass

    def close(self) -> None:
        pass
