"""Breach onset per service on the host: the rules of the breach-onset tracker.

Every other reduction is per window: the finest time known for a fault is the window it first scored
in, and a breach exported late counts in the window it arrives in. This tracker bins the counted span
records by their own start time (``ts_ns``) and runs a CUSUM over the bins, so it can say **when** the
current run of breaches began -- and a late record revises the past.

**Which records count**: the sketch's observed set. A 64-byte SPAN without SPAN_NO_SLI, with
``group_id < n_groups`` (else ``out_of_group``) and ``ttft_ms >= 0`` in a float32 compare (else
``invalid``). **Breach**: ``ttft_ms > slo_ms`` in float32. An observed record with ``ts_ns <= 0`` goes
to ``no_time`` and into no bin.

**Bins**: ``q = ts_ns // bin_ns`` is the absolute bin. Every service has a ring of ``B`` bins (a power
of two), slot ``q & (B - 1)``. A step carries its cut's time: ``q_hi = max(previous q_hi, cut_ns //
bin_ns)`` never moves back (-1 before the first step), the ring covers ``q_hi - B < q <= q_hi``.
Before observing, the slots of the bins ``(previous q_hi, q_hi]`` are cleared in every row (a jump of
``B`` or more clears everything). A record with ``q > q_hi`` (a service clock ahead of the agent) is
placed in ``q_hi`` and counted in ``future``; one with ``q <= q_hi - B`` is counted in ``too_old`` and
placed nowhere.

**Cell**: one u64 per (service, slot): ``cell += (breach << 32) | 1``.

**The bound that keeps it exact**: the tracker keeps (``q_hi`` of the step, spans offered) of every
step, drops those with ``q_hi <= current q_hi - B`` (their records are all cleared) and refuses a
step, before anything changes, when the rest plus the step's spans would exceed ``ring_records_max``
(at most 2^31 - 1). Under it no cell's low word carries and every CUSUM quantity stays below 2^52.

**CUSUM**: per bin ``x = b * 1_000_000 - n * ref_ppm`` (int64); from the ring's oldest bin to
``q_hi``: ``S_t = max(0, S_{t-1} + x_t)``, 0 before the oldest bin. Threshold ``h = alarm * 1_000_000``.

**Per service** (``ONSET_ROW``, 64 bytes): ``state`` (0 quiet, 1 excursion, 2 alarm = the open
excursion has reached ``h``), ``flags`` (bit 0 ``clipped``: no zero of ``S`` in the ring), ``onset_q``
(1 + the last bin with ``S == 0``; the ring's oldest bin when clipped; -1 when quiet, i.e. ``S`` at
``q_hi`` is 0), ``alarm_q`` (the first bin >= ``onset_q`` with ``S >= h``, or -1), ``s_now`` / ``s_peak``
(``S`` at ``q_hi``, its maximum since ``onset_q``), ``n_exc`` / ``b_exc`` (requests and breaches since
``onset_q``), ``n_ring`` / ``b_ring`` (in the whole ring). Times are ``q * bin_ns``. Nothing but the ring
is kept between steps: the rows are a pure function of the ring and the parameters.

``OnsetOracle`` is the rules in numpy: the reference the device tracker (ops/csrc/onset.hip,
ops/onset.py) is tested against for equality, and what ``engine="cpu"`` uses. ``scan_rows`` computes
the CUSUM the way the device does (runs of bins under ``combine``), ``sequential_rows`` by the
recurrence; both are kept equal by tests/test_onset.py.
"""

from __future__ import annotations

from collections import deque
from typing import Deque, Dict, Sequence, Tuple

import numpy as np

from ..collector import records
from .trackerstate import OracleCheckpoint

MIN_BINS, MAX_BINS = 64, 8192
MIN_BIN_NS, MAX_BIN_NS = 1_000_000, 60_000_000_000
MILLION = 1_000_000
MAX_RING_RECORDS = (1 << 31) - 1
ROW_BYTES = 64
NO_BIN = -1
QUIET, EXCURSION, ALARM = 0, 1, 2
CLIPPED = 1
# one service (ops/csrc/onset_host.h Row)
ONSET_ROW = np.dtype([("state", "<u4"), ("flags", "<u4"), ("onset_q", "<i8"), ("alarm_q", "<i8"), ("s_now", "<i8"),
                      ("s_peak", "<i8"), ("n_exc", "<u4"), ("b_exc", "<u4"), ("n_ring", "<u4"), ("b_ring", "<u4"),
                      ("pad", "<u4", (2,))])
assert ONSET_ROW.itemsize == ROW_BYTES
# per-step statistics, in the device's order (ops/csrc/onset_host.h Stat)
STATS = ("observed", "invalid", "out_of_group", "no_time", "future", "too_old")
N_STATS = 8
EVENT_STATS = ("invalid", "out_of_group", "no_time", "future", "too_old")
RESULT_FIELDS = ("rows", "stats")
# what WindowPipeline.results() gains with the tracker on
RESULT_KEYS = ("onset_rows",)


def stats_dict(stats: np.ndarray) -> Dict[str, int]:
    return {name: int(stats[i]) for i, name in enumerate(STATS)}


def result_keys(result: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """A step's results under the names WindowPipeline.results() carries (RESULT_KEYS)."""
    return {"onset_rows": np.asarray(result["rows"])}


def quiet_rows(n: int) -> np.ndarray:
    rows = np.zeros(int(n), ONSET_ROW)
    rows["onset_q"] = NO_BIN
    rows["alarm_q"] = NO_BIN
    return rows


def empty_result(n_groups: int) -> Dict[str, np.ndarray]:
    """A window the tracker did not step for: quiet rows over an empty ring, no statistics."""
    return {"rows": quiet_rows(n_groups), "stats": np.zeros(N_STATS, np.uint32)}


# ---- bins (ops/csrc/onset_host.h) ---------------------------------------------------------------
def bin_of(ts_ns: int, bin_ns: int) -> int:
    return int(ts_ns) // int(bin_ns)


def slot_of(q: int, bins: int) -> int:
    return int(q) & (int(bins) - 1)


def oldest_bin(q_hi: int, bins: int) -> int:
    return int(q_hi) - int(bins) + 1


def advance(q_hi: int, cut_ns: int, bin_ns: int) -> int:
    return max(int(q_hi), bin_of(cut_ns, bin_ns))


def cleared(prev: int, q_hi: int, bins: int) -> int:
    return min(int(bins), int(q_hi) - int(prev))


def combine(a: Tuple[int, int], b: Tuple[int, int]) -> Tuple[int, int]:
    """Runs of bins as (sum, minimum inclusive prefix capped at 0): ``a`` then ``b``."""
    return a[0] + b[0], min(a[1], a[0] + b[1])


def run_of(x: int) -> Tuple[int, int]:
    return int(x), min(int(x), 0)


def lds_key(g: int, slot: int) -> int:
    return ((int(g) + 1) << 16) | int(slot)


def lds_hash(key: int) -> int:
    """The first slot the observe kernel probes in its 256-slot LDS table."""
    return ((int(key) * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)) >> 56


def layout_words(group_cap: int) -> int:
    return (int(group_cap) * (ROW_BYTES // 4) + N_STATS + 3) & ~3


def device_bytes(bins: int, span_cap: int, group_cap: int) -> int:
    """ops/csrc/onset_host.h device_bytes()."""
    return int(span_cap) * 64 + int(group_cap) * int(bins) * 8 + layout_words(group_cap) * 4


def check_config(bins: int, bin_ns: int, ref_ppm: int, alarm: int, span_cap: int, group_cap: int, n_buffers: int,
                 slo_ms: float, ring_records_max: int = MAX_RING_RECORDS) -> None:
    """The configuration checks of ops/csrc/onset_host.h validate()."""
    if not MIN_BINS <= bins <= MAX_BINS or bins & (bins - 1):
        raise ValueError("breach onset: bins must be a power of two in [64, 8192]")
    if not MIN_BIN_NS <= bin_ns <= MAX_BIN_NS:
        raise ValueError("breach onset: bin_ns must be in [1000000, 60000000000]")
    if not 1 <= ref_ppm <= MILLION - 1:
        raise ValueError("breach onset: ref_ppm must be in [1, 999999]")
    if not 1 <= alarm <= MILLION:
        raise ValueError("breach onset: alarm must be in [1, 1000000]")
    if not 1 <= group_cap <= 65536:
        raise ValueError("breach onset: group_cap must be in [1, 65536]")
    if span_cap < 1:
        raise ValueError("breach onset: span_cap must be >= 1")
    if not 1 <= n_buffers <= 64:
        raise ValueError("breach onset: n_buffers out of range")
    if not (np.isfinite(slo_ms) and slo_ms >= 0):
        raise ValueError("breach onset: slo_ms must be finite and >= 0")
    if device_bytes(bins, span_cap, group_cap) > 1 << 31:
        raise ValueError("breach onset: the ring needs more than 2 GiB")
    if not 1 <= ring_records_max <= MAX_RING_RECORDS:
        raise ValueError("breach onset: ring_records_max must be in [1, 2^31 - 1]")


def ref_ppm_of(ref_burn: float, slo_target: float) -> int:
    """The reference breach rate, in millionths, of a burn rate against an SLO target: ``ref_burn``
    times the error budget ``1 - slo_target``, clamped to the valid range."""
    return int(min(MILLION - 1, max(1, round(float(ref_burn) * (1.0 - float(slo_target)) * 1e6))))


def _gather(ranges) -> np.ndarray:
    from .cpu import _gather as g

    b = g(ranges)
    return b.view(records.SPAN) if len(b) else np.zeros(0, records.SPAN)


def ordered(cells: np.ndarray, q_hi: int) -> np.ndarray:
    """The ring's cells [C, B] (slot order) in ring order: column 0 = the oldest bin."""
    B = cells.shape[1]
    return cells[:, (np.arange(B, dtype=np.int64) + oldest_bin(q_hi, B)) & (B - 1)]


def _row(n, b, q0: int, h: int, S) -> np.ndarray:
    """One service's row from its bins' S (ring order), by the rules' words."""
    row = quiet_rows(1)[0]
    row["n_ring"], row["b_ring"] = int(n.sum()), int(b.sum())
    if S[-1] == 0:
        return row
    zeros = np.nonzero(np.asarray(S) == 0)[0]
    first = int(zeros[-1]) + 1 if len(zeros) else 0
    since = np.asarray(S[first:])
    hit = np.nonzero(since >= h)[0]
    row["state"] = ALARM if len(hit) else EXCURSION
    row["flags"] = 0 if len(zeros) else CLIPPED
    row["onset_q"] = q0 + first
    row["alarm_q"] = q0 + first + int(hit[0]) if len(hit) else NO_BIN
    row["s_now"], row["s_peak"] = int(S[-1]), int(since.max())
    row["n_exc"], row["b_exc"] = int(n[first:].sum()), int(b[first:].sum())
    return row


def _split(cells: np.ndarray, q_hi: int, ref_ppm: int):
    o = ordered(np.asarray(cells, np.uint64), q_hi)
    n = (o & np.uint64(0xFFFFFFFF)).astype(np.int64)
    b = (o >> np.uint64(32)).astype(np.int64)
    return n, b, b * MILLION - n * int(ref_ppm)


def sequential_rows(cells: np.ndarray, q_hi: int, ref_ppm: int, alarm: int) -> np.ndarray:
    """The rows by the recurrence S_t = max(0, S_{t-1} + x_t), vectorised over the services."""
    n, b, x = _split(cells, q_hi, ref_ppm)
    C, B = x.shape
    S = np.zeros((C, B), np.int64)
    s = np.zeros(C, np.int64)
    for t in range(B):
        s = np.maximum(0, s + x[:, t])
        S[:, t] = s
    q0, h = oldest_bin(q_hi, B), int(alarm) * MILLION
    return np.array([_row(n[g], b[g], q0, h, S[g]) for g in range(C)], ONSET_ROW).reshape(C)


def scan_rows(cells: np.ndarray, q_hi: int, ref_ppm: int, alarm: int) -> np.ndarray:
    """The rows the way the device computes S: P_t - min(0, min P) from prefix sums (what the wave's
    scan of runs under ``combine`` yields)."""
    n, b, x = _split(cells, q_hi, ref_ppm)
    C, B = x.shape
    P = np.cumsum(x, axis=1)
    S = P - np.minimum(0, np.minimum.accumulate(P, axis=1))
    q0, h = oldest_bin(q_hi, B), int(alarm) * MILLION
    return np.array([_row(n[g], b[g], q0, h, S[g]) for g in range(C)], ONSET_ROW).reshape(C)


class OnsetOracle(OracleCheckpoint):
    """The tracker's rules in numpy (see the module docstring), with the device handle's interface."""

    # checkpoint (pipeline/trackerstate.py): the fields ops/csrc/onset_host.h fingerprint() covers, and what is
    # kept between steps
    KIND = "breach onset"
    FINGERPRINT = ("group_cap", "bins", "bin_ns", "ref_ppm", "alarm", "slo_ms", "ring_records_max")
    STATE = ("cells", "q_hi", "held", "n")

    def __init__(self, bins: int = 1024, bin_ns: int = 125_000_000, ref_ppm: int = 20000, alarm: int = 3,
                 span_cap: int = 16384, group_cap: int = 64, n_buffers: int = 3, slo_ms: float = 800.0,
                 ring_records_max: int = MAX_RING_RECORDS, device: int = 0, lds: bool = True):
        bins, bin_ns, ref_ppm, alarm = int(bins), int(bin_ns), int(ref_ppm), int(alarm)
        span_cap, group_cap, n_buffers, slo_ms = int(span_cap), int(group_cap), int(n_buffers), float(slo_ms)
        check_config(bins, bin_ns, ref_ppm, alarm, span_cap, group_cap, n_buffers, slo_ms, int(ring_records_max))
        self.bins, self.bin_ns, self.ref_ppm, self.alarm = bins, bin_ns, ref_ppm, alarm
        self.span_cap, self.group_cap, self.nb, self.slo_ms = span_cap, group_cap, n_buffers, slo_ms
        self.ring_records_max = int(ring_records_max)
        self.cells = np.zeros((group_cap, bins), np.uint64)  # slot order
        self.q_hi = NO_BIN
        self.held: Deque[Tuple[int, int]] = deque()  # (q_hi of the step, spans offered)
        self.res: Dict[int, Tuple[int, dict]] = {}
        self.n = 0

    # ---- one window ---------------------------------------------------------------------------
    def step(self, span_ranges: Sequence[Tuple[int, int]], cut_ns: int, n_groups: int) -> int:
        """``span_ranges`` = [(host address, bytes)] of 64-byte SPAN records, as the engine gets them."""
        for _a, nbytes in span_ranges:
            if int(nbytes) % 64:
                raise ValueError("breach onset step: a range is not whole 64-byte spans")
        return self.step_records(_gather(span_ranges), cut_ns, n_groups)

    def population_after(self, q_hi: int, n: int) -> int:
        return int(n) + sum(c for q, c in self.held if q > q_hi - self.bins)

    def step_records(self, spans: np.ndarray, cut_ns: int, n_groups: int) -> int:
        G, C, B = int(n_groups), self.group_cap, self.bins
        if int(cut_ns) <= 0:
            raise ValueError("breach onset step: cut_ns must be > 0")
        if not 0 <= G <= C:
            raise ValueError("breach onset step: n_groups out of range")
        if len(spans) > self.span_cap:
            raise ValueError("breach onset step: more spans than span_cap")
        prev, q_hi = self.q_hi, advance(self.q_hi, cut_ns, self.bin_ns)
        if self.population_after(q_hi, len(spans)) > self.ring_records_max:
            raise ValueError("breach onset step: the ring would hold more than ring_records_max spans")
        # nothing has changed up to here
        while self.held and self.held[0][0] <= q_hi - B:
            self.held.popleft()
        if len(spans):
            self.held.append((q_hi, len(spans)))
        self.q_hi = q_hi
        if q_hi > prev:
            self.cells[:, (prev + 1 + np.arange(cleared(prev, q_hi, B), dtype=np.int64)) & (B - 1)] = 0

        grp = spans["group_id"].astype(np.int64)
        v = np.ascontiguousarray(spans["ttft_ms"], dtype=np.float32)
        sli = (spans["flags"] & np.uint32(records.SPAN_NO_SLI)) == 0
        counts = sli & (grp < G)
        with np.errstate(invalid="ignore"):
            ok = counts & (v >= np.float32(0.0))
        at = np.nonzero(ok)[0]
        g, ts, x = grp[at], spans["ts_ns"][at].astype(np.int64), v[at]
        timed = ts > 0
        q = ts // self.bin_ns
        future = timed & (q > q_hi)
        old = timed & (q <= q_hi - B)
        placed = timed & ~old
        q = np.where(future, q_hi, q)
        add = (x > np.float32(self.slo_ms)).astype(np.uint64) << np.uint64(32) | np.uint64(1)
        np.add.at(self.cells, (g[placed], q[placed] & (B - 1)), add[placed])
        stats = np.zeros(N_STATS, np.uint32)
        stats[:len(STATS)] = [len(at), int((counts & ~ok).sum()), int((sli & (grp >= G)).sum()), int((~timed).sum()),
                              int(future.sum()), int(old.sum())]

        idx = self.n
        self.res[idx % self.nb] = (idx, {"rows": scan_rows(self.cells, q_hi, self.ref_ppm, self.alarm), "stats": stats})
        self.n += 1
        return idx

    # ---- results ------------------------------------------------------------------------------
    def query(self, i: int) -> bool:
        return True

    def _held(self, i: int):
        held = self.res.get(int(i) % self.nb)
        if held is None or held[0] != int(i):
            raise IndexError(f"breach onset step {i} is not held (only the last {self.nb})")
        return held

    def results(self, i: int, n_groups: int) -> Dict[str, np.ndarray]:
        held = self._held(i)
        G = int(n_groups)
        if not 0 <= G <= self.group_cap:
            raise ValueError("n_groups")
        return {"rows": held[1]["rows"][:G].copy(), "stats": held[1]["stats"].copy()}

    def step_ms(self, i: int) -> Tuple[float, float]:
        return 0.0, 0.0

    def resident(self) -> Dict[str, np.ndarray]:
        """The whole ring: ``n`` / ``b`` [group_cap, B] in slot order, and ``q_hi``."""
        return {"n": (self.cells & np.uint64(0xFFFFFFFF)).astype(np.uint32),
                "b": (self.cells >> np.uint64(32)).astype(np.uint32), "q_hi": int(self.q_hi)}

    def sync(self) -> None:
        pass

    def close(self) -> None:
        pass
