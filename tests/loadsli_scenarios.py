"""Span windows for the load SLI tests (pipeline/loadsli.py, ops/loadsli.py): builders of finishing
records with a start and a duration, the named cases both test files run (CASES), and the brute force
the oracle is checked against -- every request kept as its interval and every bin of the ring computed
from the intervals themselves (who touches it, how long inside it), no cells, no idle time, no carry,
no prefix sums."""

from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.pipeline import loadsli as ld

F32 = np.float32
BIN = 1000                              # 1 ms bins, in microseconds
T0_US = 1_700_000_000_000_000           # a bin edge: T0_US % BIN == 0
Q0 = T0_US // BIN
SETTLE, RECENT, MIN_BASE = 2, 4, 8
DAY_MS = 86_400_000.0
NOT_AN_END = R.SPAN_START | R.SPAN_FIRST_TOKEN
# dur_us on boundary bit patterns (latency_ms as float32 -> whole microseconds)
DUR_PATTERNS = [(0.0, 0), (1e-4, 0), (0.9995, 999), (1.0005, 1000), (799.9999, 799999), (3.3333333, 3333),
                (86_400_000.0, 86_400_000_000)]


def reqs(grp: Sequence[int], start_us: Sequence[int], dur_ms: Sequence[float], flags=0, ns: int = 0) -> np.ndarray:
    """Finishing records: service, start in microseconds (``ns`` more nanoseconds), duration in ms."""
    n = len(grp)
    r = np.zeros(n, dtype=R.SPAN)
    r["group_id"] = np.asarray(grp, dtype=np.uint32)
    r["ts_ns"] = np.asarray(start_us, dtype=np.int64) * 1000 + ns
    r["latency_ms"] = np.asarray(dur_ms, dtype=F32)
    r["ttft_ms"] = F32(np.nan)  # must not matter
    r["flags"] = flags
    r["trace_h"] = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    return r


def req(g: int, q: int, off_us: int, dur_ms: float, flags=0, ns: int = 0) -> np.ndarray:
    """One request of service g starting ``off_us`` into bin q."""
    return reqs([g], [q * BIN + off_us], [dur_ms], flags, ns)


def cat(*parts: np.ndarray) -> np.ndarray:
    return np.concatenate(parts) if parts else np.zeros(0, R.SPAN)


EMPTY = np.zeros(0, R.SPAN)


def traffic(g: int, q_from: int, q_to: int, per_bin: int, dur_ms: float) -> np.ndarray:
    """``per_bin`` requests of service g in every bin of [q_from, q_to], evenly spaced from the bin's edge."""
    qs = np.repeat(np.arange(q_from, q_to + 1, dtype=np.int64), per_bin)
    off = np.tile(np.arange(per_bin, dtype=np.int64) * (BIN // max(per_bin, 1)), q_to - q_from + 1)
    return reqs([g] * len(qs), qs * BIN + off, [dur_ms] * len(qs))


def cut_of(q: int) -> int:
    """A cut inside bin q, ns."""
    return (q * BIN + BIN // 2) * 1000


# ---- the brute force ----------------------------------------------------------------------------
class Brute:
    """The rules request by request: every placed request is kept as (service, ts_us, te_us, qe) -- after
    the moves the placement makes for a clock ahead of the agent; qe is te_us // bin_us but for a
    request cut at the end of q_hi, which ends in q_hi -- and every bin of the ring is computed from
    the intervals: active = the requests with qs <= t <= qe, busy = the sum of their overlaps with the
    bin, arrivals = those with qs == t, completions = those with qe == t."""

    def __init__(self, bins, bin_us, settle_bins, recent_bins, min_base_bins, factor_milli, min_requests, min_conc_milli,
                 group_cap, **_kw):
        self.B, self.bin, self.C = bins, bin_us, group_cap
        self.settle, self.R, self.min_base = settle_bins, recent_bins, min_base_bins
        self.f, self.min_requests, self.min_conc = factor_milli, min_requests, min_conc_milli
        self.reqs: List[Tuple[int, int, int, int]] = []
        self.q_hi = self.q_first = -1
        self.age = [0] * group_cap
        self.prev = [0] * group_cap

    def step(self, recs: np.ndarray, cut_ns: int, n_groups: int) -> Dict[str, np.ndarray]:
        prev, B, bin_us = self.q_hi, self.B, self.bin
        self.q_hi = q_hi = max(self.q_hi, (cut_ns // 1000) // bin_us)
        if prev == -1 or q_hi - prev >= B:
            self.q_first = q_hi
        oldest = q_hi - B + 1
        stats = dict.fromkeys(ld.STATS, 0)
        for r in recs:
            if int(r["flags"]) & NOT_AN_END:
                continue
            g, v, ts_ns = int(r["group_id"]), F32(r["latency_ms"]), int(r["ts_ns"])
            if g >= n_groups:
                stats["out_of_group"] += 1
                continue
            if not (v >= F32(0) and v <= F32(DAY_MS)):
                stats["invalid"] += 1
                continue
            if ts_ns <= 0:
                stats["no_time"] += 1
                continue
            stats["observed"] += 1
            ts = ts_ns // 1000
            dur = int(float(v) * 1000.0)  # a Python float is an IEEE double; int() truncates
            te = ts + dur
            qe = te // bin_us
            if dur > self.settle * bin_us:
                stats["long"] += 1
            if ts // bin_us > q_hi:
                stats["future"] += 1
                ts = te = q_hi * bin_us
                qe = q_hi
            elif qe > q_hi:
                stats["future"] += 1
                te = (q_hi + 1) * bin_us
                qe = q_hi
            if qe < oldest:
                stats["too_old"] += 1
                continue
            if ts // bin_us < oldest:
                stats["clipped"] += 1
            self.reqs.append((g, ts, te, qe))
        st = np.array([stats[name] for name in ld.STATS], np.uint32)
        return {"rows": self.rows(), "stats": st}

    def bins_of(self, g: int):
        """(arrivals, completions, active, busy, in flight after) per bin of the ring, oldest first."""
        B, bin_us, oldest = self.B, self.bin, self.q_hi - self.B + 1
        mine = np.array([(ts, te, qe) for s, ts, te, qe in self.reqs if s == g], np.int64).reshape(-1, 3)
        ts, te, qe = mine[:, 0][:, None], mine[:, 1][:, None], mine[:, 2][:, None]
        lo = ((oldest + np.arange(B, dtype=np.int64)) * bin_us)[None, :]
        hi = lo + bin_us
        qs, t = ts // bin_us, lo // bin_us
        arr = (qs == t).sum(axis=0)
        done = (qe == t).sum(axis=0)
        active = ((qs <= t) & (t <= qe)).sum(axis=0)
        busy = np.clip(np.minimum(te, hi) - np.maximum(ts, lo), 0, None).sum(axis=0)
        after = ((qs <= t) & (qe > t)).sum(axis=0)
        return arr, done, active, busy, after

    def rows(self) -> np.ndarray:
        out = ld.warming_rows(self.C)
        q_hi, oldest = self.q_hi, self.q_hi - self.B + 1
        lo = max(oldest, self.q_first)
        rec_hi = q_hi - self.settle
        rec_lo = rec_hi - self.R + 1
        nb = max(0, rec_lo - lo)
        warming = rec_lo < lo or nb < self.min_base
        for g in range(self.C):
            arr, done, active, busy, after = self.bins_of(g)
            assert (after >= 0).all() and after[-1] == 0  # every observed request has finished
            row = out[g]
            row["busy_ring"], row["arr_ring"], row["peak_active"] = busy.sum(), arr.sum(), active.max()
            peak_at = [i for i in range(self.B) if active[i] == active.max()][0]
            row["peak_q"] = oldest + peak_at if active.max() > 0 else -1
            state = ld.WARMING
            if not warming:
                r = slice(rec_lo - oldest, rec_hi - oldest + 1)
                b = slice(lo - oldest, rec_lo - oldest)
                row["busy_recent"], row["busy_base"] = busy[r].sum(), busy[b].sum()
                row["arr_recent"], row["arr_base"] = arr[r].sum(), arr[b].sum()
                row["done_recent"], row["done_base"] = done[r].sum(), done[b].sum()
                row["base_bins"] = nb
                flags, state = ld.classify(int(busy[r].sum()), int(busy[b].sum()), int(arr[r].sum()), int(arr[b].sum()), nb,
                                           self.R, self.bin, self.f, self.min_requests, self.min_conc)
                row["flags"], row["state"] = flags, state
            if 1 <= state <= 3:
                self.age[g] = min(self.age[g] + 1, 2 ** 32 - 1) if self.prev[g] == state else 1
            else:
                self.age[g] = 0
            self.prev[g] = state
            row["age"] = self.age[g]
        return out


def same_rows(a: np.ndarray, b: np.ndarray, what: str = "") -> None:
    """Rows compared as bytes."""
    assert a.dtype == b.dtype == ld.LOAD_ROW and a.shape == b.shape, (what, a.dtype, a.shape, b.shape)
    if np.ascontiguousarray(a).tobytes() != np.ascontiguousarray(b).tobytes():
        raise AssertionError(f"{what}: rows differ\n{a}\n{b}")


def same_results(a: dict, b: dict, what: str = "") -> None:
    assert set(a) == set(b) == set(ld.RESULT_FIELDS), what
    same_rows(a["rows"], b["rows"], what)
    assert a["stats"].dtype == b["stats"].dtype == np.uint32 and a["stats"].shape == b["stats"].shape == (ld.N_STATS,)
    np.testing.assert_array_equal(a["stats"], b["stats"], err_msg=f"{what} stats")


RESIDENT = (("counts", np.uint64), ("idle_us", np.uint64), ("carry", np.int32), ("age", np.uint32), ("prev_state", np.uint32))


def same_resident(a: dict, b: dict, what: str = "") -> None:
    assert (int(a["q_hi"]), int(a["q_first"])) == (int(b["q_hi"]), int(b["q_first"])), (what, a["q_hi"], b["q_hi"])
    for f, dt in RESIDENT:
        assert a[f].dtype == b[f].dtype == dt and a[f].shape == b[f].shape, (what, f, a[f].dtype, b[f].dtype)
        np.testing.assert_array_equal(a[f], b[f], err_msg=f"{what} resident {f}")


# ---- the named cases ----------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    cfg: dict
    steps: List[Tuple[np.ndarray, int, int]]          # (records, cut_ns, n_groups)
    # over every step's results (all rows of group_cap; None for a refused step) and resident state
    check: Optional[Callable[[List[Optional[dict]], List[dict]], None]] = None
    refused: Tuple[int, ...] = ()                     # steps that must be refused, changing nothing


def _cfg(bins=64, group_cap=3, span_cap=256, f=1500, min_requests=4, min_conc_milli=500, **kw):
    return dict(bins=bins, bin_us=BIN, settle_bins=SETTLE, recent_bins=RECENT, min_base_bins=MIN_BASE, factor_milli=f,
                min_requests=min_requests, min_conc_milli=min_conc_milli, group_cap=group_cap, span_cap=span_cap, **kw)


def _stat(res, name):
    return int(res["stats"][ld.STATS.index(name)])


QH = Q0 + 100  # the single cut of the one-step cases


def _one(name, recs, check, G=3, bins=64, **kw) -> Case:
    return Case(name, _cfg(bins, **kw), [(recs, cut_of(QH), G)], check)


def _geometry() -> List[Case]:
    q = QH - 20

    def row_is(busy, peak_q, arr=1, peak=1, ends_slot=None):
        def check(res, resid):
            row = res[-1]["rows"][1]
            assert (int(row["busy_ring"]), int(row["arr_ring"]), int(row["peak_active"]), int(row["peak_q"])) == \
                (busy, arr, peak, peak_q)
            assert _stat(res[-1], "observed") == arr and int(row["state"]) == ld.WARMING and int(row["base_bins"]) == 0
            if ends_slot is not None:
                assert int(resid[-1]["counts"][1, ends_slot & 63]) >> 32 == 1
        return check

    return [_one("inside one bin", req(1, q, 100, 0.5, ns=999), row_is(500, q)),
            _one("over three bins", req(1, q, 600, 2.0), row_is(2000, q, ends_slot=q + 2)),
            _one("ending on a bin boundary", req(1, q, 500, 0.5), row_is(500, q, ends_slot=q + 1)),
            _one("zero duration", req(1, q, 250, 0.0), row_is(0, q, ends_slot=q)),
            _one("two in a bin, one spanning", cat(req(1, q, 0, 0.25), req(1, q, 900, 1.25), req(1, q + 1, 10, 0.125)),
                 row_is(250 + 1250 + 125, q, arr=3, peak=2))]


def _placement() -> List[Case]:
    oldest = QH - 63

    def stats_are(**want):
        def check(res, resid):
            got = ld.stats_dict(res[-1]["stats"])
            assert got == dict(dict.fromkeys(ld.STATS, 0), **want), got
        return check

    def clipped(res, resid):
        stats_are(observed=1, clipped=1, long=1)(res, resid)
        row = res[-1]["rows"][0]
        assert int(resid[-1]["carry"][0]) == 1 and int(row["arr_ring"]) == 0
        # in flight from the ring's oldest bin to its end, 3.5 bins later
        assert int(row["busy_ring"]) == 3500 and int(row["peak_active"]) == 1 and int(row["peak_q"]) == oldest

    def future_start(res, resid):
        stats_are(observed=1, future=1)(res, resid)
        row = res[-1]["rows"][0]
        assert (int(row["arr_ring"]), int(row["busy_ring"]), int(row["peak_q"])) == (1, 0, QH)
        assert int(resid[-1]["idle_us"][0, QH & 63]) == BIN and int(resid[-1]["counts"][0, QH & 63]) == (1 << 32) | 1

    def future_end(res, resid):
        stats_are(observed=1, future=1, long=1)(res, resid)
        row = res[-1]["rows"][0]
        assert (int(row["arr_ring"]), int(row["busy_ring"]), int(row["peak_q"])) == (1, 2 * BIN - 300, QH - 1)

    above_a_day = float(np.nextafter(F32(DAY_MS), F32(np.inf)))
    flags_that_do_not_matter = R.SPAN_NO_SLI | R.SPAN_LATE | R.pack_outcome(5) | R.pack_tpot_us(1234)
    return [
        _one("clipped", req(0, oldest - 7, 500, 10.0), clipped),
        _one("too old", cat(req(0, oldest - 7, 500, 6.0), req(0, oldest - 1, 0, 0.999)), stats_are(observed=2, too_old=2, long=1)),
        _one("ending in the oldest bin", req(0, oldest - 1, 999, 0.001), stats_are(observed=1, clipped=1)),
        _one("a future start", req(0, QH + 3, 10, 1.0), future_start),
        _one("a future end", req(0, QH - 1, 300, 5.0), future_end),
        _one("no time", cat(reqs([0, 1], [0, -5], [1.0, 1.0]), req(2, QH - 9, 0, 0.5)), stats_are(observed=1, no_time=2)),
        _one("invalid latencies", reqs([0] * 6, [(QH - 9) * BIN] * 6, [np.nan, -1.0, np.inf, above_a_day, -np.inf, -0.0]),
             stats_are(observed=1, invalid=5)),
        _one("a day long", reqs([0], [QH * BIN - 86_400_000_000 + 3], [DAY_MS]), stats_are(observed=1, clipped=1, long=1)),
        _one("out of group", reqs([2, 3, 700, 1], [(QH - 9) * BIN] * 4, [0.5] * 4), stats_are(observed=1, out_of_group=3), G=2),
        _one("start and first-token records skipped",
             cat(req(0, QH - 9, 0, 0.5, R.SPAN_START | R.SPAN_NO_SLI), req(0, QH - 9, 0, 0.5, R.SPAN_FIRST_TOKEN),
                 req(7, QH - 9, 0, np.nan, R.SPAN_FIRST_TOKEN | R.SPAN_LATE), req(1, QH - 9, 0, 0.5)), stats_are(observed=1)),
        _one("a no-sli finishing record observed", req(0, QH - 9, 0, 0.5, flags_that_do_not_matter), stats_are(observed=1)),
        _one("the long statistic", cat(req(0, QH - 9, 0, 2.0), req(0, QH - 9, 0, 2.002), req(0, QH - 9, 0, 2.5)),
             stats_are(observed=3, long=2)),
    ]


def _advance() -> List[Case]:
    B = 64
    q = Q0 + 200

    def win(qh, g=0):
        return cat(traffic(g, qh - 6, qh - 3, 2, 0.25), req(1, qh - 4, 100, 1.5))

    def moves(expect):
        def check(res, resid):
            assert [(r["q_hi"], r["q_first"]) for r in resid] == expect
        return check

    several = [(win(q), cut_of(q), 2), (win(q), cut_of(q), 2), (win(q + 1), cut_of(q + 1), 2), (win(q + 6), cut_of(q + 6), 2)]
    back = [(win(q + 10), cut_of(q + 10), 2), (win(q + 3), cut_of(q + 3), 2), (EMPTY, 1000, 2), (win(q + 11), cut_of(q + 11), 2)]
    # enough history to leave warming, then a jump of exactly B and one of more than B
    jump = [(EMPTY, cut_of(q), 2), (traffic(0, q, q + 18, 2, 0.25), cut_of(q + 20), 2),
            (win(q + 20 + B), cut_of(q + 20 + B), 2), (win(q + 21 + B), cut_of(q + 21 + B), 2),
            (win(q + 400), cut_of(q + 400), 2)]

    def jumped(res, resid):
        moves([(q, q), (q + 20, q), (q + 20 + B, q + 20 + B), (q + 21 + B, q + 20 + B), (q + 400, q + 400)])(res, resid)
        assert [int(r["rows"]["state"][0]) for r in res] == [4, 0, 4, 4, 4]
        assert all(int(r["carry"].sum()) == 0 for r in resid)

    return [Case("advance by 0, 1 and several bins", _cfg(B), several, moves([(q, q), (q, q), (q + 1, q), (q + 6, q)])),
            Case("a cut moving back", _cfg(B), back, moves([(q + 10, q + 10)] * 3 + [(q + 11, q + 10)])),
            Case("advance by B or more", _cfg(B), jump, jumped)]


def _ring() -> List[Case]:
    B = 64
    q = Q0 + 300

    def late(res, resid):
        a, b = res[0]["rows"][0], res[1]["rows"][0]
        assert int(a["arr_ring"]) == 2 and int(b["arr_ring"]) == 5 and int(b["busy_ring"]) == int(a["busy_ring"]) + 3 * 2500
        assert (int(a["peak_active"]), int(a["peak_q"])) == (1, q - 8) and (int(b["peak_active"]), int(b["peak_q"])) == (3, q - 12)

    late_case = Case("a late record landing in past bins", _cfg(B),
                     [(cat(req(0, q - 8, 0, 0.5), req(0, q - 5, 0, 0.5)), cut_of(q), 1),
                      (reqs([0] * 3, [(q - 12) * BIN + 100 * i for i in range(3)], [2.5] * 3), cut_of(q + 16), 1)], late)

    # starts in q - 2, ends in q + 38: observed whole; the start is evicted first (carry 1), then the end (carry 0)
    evict = Case("start evicted while the end is in the ring", _cfg(B),
                 [(req(1, q - 2, 250, 40.0), cut_of(q + 40), 2), (EMPTY, cut_of(q + 70), 2), (EMPTY, cut_of(q + 101), 2),
                  (EMPTY, cut_of(q + 102), 2)])

    def evicted(res, resid):
        assert [int(r["carry"][1]) for r in resid] == [0, 1, 1, 0]
        assert [int(r["rows"]["arr_ring"][1]) for r in res] == [1, 0, 0, 0]
        # the ring's oldest bin is q + 7, then q + 38 (the end's own bin: 250 us of it), then past the end
        assert [int(r["rows"]["busy_ring"][1]) for r in res] == [40000, (q + 38 - (q + 7)) * BIN + 250, 250, 0]
        assert [int(r["rows"]["peak_q"][1]) for r in res] == [q - 2, q + 7, q + 38, -1]

    evict = evict._replace(check=evicted)

    def tie(B_, idx_a, idx_b, name):
        qh = q + 500
        oldest = qh - B_ + 1
        recs = cat(traffic(2, oldest + idx_b, oldest + idx_b, 3, 0.125), traffic(2, oldest + idx_a, oldest + idx_a, 3, 0.125),
                   traffic(2, oldest + idx_a + 5, oldest + idx_a + 5, 2, 0.125))

        def check(res, resid):
            row = res[-1]["rows"][2]
            assert (int(row["peak_active"]), int(row["peak_q"])) == (3, oldest + min(idx_a, idx_b))

        return Case(name, _cfg(B_), [(recs, cut_of(qh), 3)], check)

    return [late_case, evict, tie(128, 40, 41, "a peak tie inside a lane's bins"), tie(128, 30, 77, "a peak tie across lanes"),
            tie(64, 9, 50, "a peak tie at one bin a lane")]


# One step that sets q_first = QF, one at QF + 13 with the records: the base is the 8 bins QF .. QF + 7,
# the recent range QF + 8 .. QF + 11, the last two bins settle.
QF = Q0 + 1000
BASE, REC = (QF, QF + 7), (QF + 8, QF + 11)


def _ranged(name, base_recs, rec_recs, want_state, want_flags, extra=None, **kw) -> Case:
    def check(res, resid):
        row = res[-1]["rows"][0]
        assert int(res[0]["rows"][0]["state"]) == ld.WARMING
        assert (int(row["state"]), int(row["flags"]), int(row["base_bins"])) == (want_state, want_flags, 8), (name, row)
        assert int(row["age"]) == (1 if 1 <= want_state <= 3 else 0)
        if extra is not None:
            extra(row)

    return Case(name, _cfg(64, **kw), [(EMPTY, cut_of(QF), 1), (cat(base_recs, rec_recs), cut_of(QF + 13), 1)], check)


def _spread(n: int, rng_: Tuple[int, int], dur_ms: float = 0.0) -> np.ndarray:
    """n requests of service 0 dealt round-robin over the bins of ``rng_``, 10 us apart inside a bin."""
    nb = rng_[1] - rng_[0] + 1
    return reqs([0] * n, [(rng_[0] + i % nb) * BIN + 10 * (i // nb) for i in range(n)], [dur_ms] * n)


def _states() -> List[Case]:
    q = QF

    def state_seq(want):
        def check(res, resid):
            assert [int(r["rows"]["state"][0]) for r in res] == want
        return check

    warm = Case("warming until min_base_bins", _cfg(64),
                [(EMPTY, cut_of(q), 1), (traffic(0, q, q + 12, 2, 0.25), cut_of(q + 12), 1), (EMPTY, cut_of(q + 13), 1),
                 (EMPTY, cut_of(q + 14), 1)], state_seq([4, 4, 0, 0]))

    def sums(**want):
        def extra(row):
            got = {k: int(row[k]) for k in want}
            assert got == want, got
        return extra

    return [
        warm,
        _ranged("steady", traffic(0, *BASE, 2, 0.25), traffic(0, *REC, 2, 0.25), ld.STEADY, 0,
                sums(arr_base=16, arr_recent=8, done_base=16, done_recent=8, busy_base=4000, busy_recent=2000)),
        _ranged("surge", traffic(0, *BASE, 2, 0.25), traffic(0, *REC, 4, 0.25), ld.SURGE, ld.ARR_UP | ld.CONC_UP),
        _ranged("slowdown", traffic(0, *BASE, 2, 0.25), traffic(0, *REC, 2, 0.75), ld.SLOWDOWN, ld.CONC_UP,
                sums(arr_base=16, arr_recent=8, busy_base=4000)),
        _ranged("drop", traffic(0, *BASE, 4, 0.125), traffic(0, *REC, 1, 0.125), ld.DROP, ld.ARR_DOWN),
    ]


def _compares() -> List[Case]:
    one_ms_a_bin = traffic(0, *BASE, 1, 1.0)  # busy_base 8000: a concurrency of 1000 thousandths
    conc_1500 = cat(traffic(0, *REC, 1, 1.0), traffic(0, *REC, 1, 0.5))  # busy_recent 6000: 1500 thousandths
    out = [
        # arr_recent * nb * 1000 = 6 * 8 * 1000 = 48000 = f * arr_base * nr = 1500 * 8 * 4
        _ranged("arr_up at equality", _spread(8, BASE), _spread(6, REC), ld.SURGE, ld.ARR_UP),
        _ranged("arr_up one below equality", _spread(8, BASE), _spread(6, REC), ld.STEADY, 0, f=1501),
        # arr_recent * nb * f = 4 * 8 * 1500 = 48000 = 1000 * arr_base * nr = 1000 * 12 * 4
        _ranged("arr_down at equality", _spread(12, BASE), _spread(4, REC), ld.DROP, ld.ARR_DOWN),
        _ranged("arr_down one below equality", _spread(12, BASE), _spread(4, REC), ld.STEADY, 0, f=1501),
        # its first compare at equality: arr_base * nr = 8 * 4 = 32 = min_requests * nb = 4 * 8
        _ranged("arr_down base rate at equality", _spread(8, BASE), EMPTY, ld.DROP, ld.ARR_DOWN),
        _ranged("arr_down base rate one below", _spread(8, BASE), EMPTY, ld.STEADY, 0, min_requests=5),
        # conc_recent * 1000 = 1500000 = f * conc_base = 1500 * 1000; min_requests out of reach for the arrival compares
        _ranged("conc_up at equality", one_ms_a_bin, conc_1500, ld.SLOWDOWN, ld.CONC_UP, min_requests=100),
        _ranged("conc_up one below equality", one_ms_a_bin, conc_1500, ld.STEADY, 0, min_requests=100, f=1501),
        _ranged("min_requests met", EMPTY, _spread(4, REC), ld.SURGE, ld.ARR_UP),
        _ranged("min_requests missed", EMPTY, _spread(4, REC), ld.STEADY, 0, min_requests=5),
        # busy_recent 2000 over 4 bins: 500 thousandths
        _ranged("min_conc_milli met", EMPTY, traffic(0, *REC, 1, 0.5), ld.SLOWDOWN, ld.CONC_UP, min_requests=100),
        _ranged("min_conc_milli missed", EMPTY, traffic(0, *REC, 1, 0.5), ld.STEADY, 0, min_requests=100, min_conc_milli=501),
        _ranged("surge takes precedence over slowdown", one_ms_a_bin, conc_1500, ld.SURGE, ld.ARR_UP | ld.CONC_UP),
    ]

    # surge (age 1, 2, 3 on standing cuts), late base records turn it into a drop (age 1, 2), then steady (0)
    cut = cut_of(QF + 13)
    steps = [(EMPTY, cut_of(QF), 1), (cat(_spread(8, BASE), _spread(8, REC)), cut, 1), (EMPTY, cut, 1), (EMPTY, cut - 1, 1),
             (_spread(64, BASE), cut, 1), (EMPTY, cut, 1), (_spread(24, REC), cut, 1), (EMPTY, cut, 1)]

    def ages(res, resid):
        assert [(int(r["rows"]["state"][0]), int(r["rows"]["age"][0])) for r in res] == \
            [(4, 0), (1, 1), (1, 2), (1, 3), (3, 1), (3, 2), (0, 0), (0, 0)]
        assert [int(r["age"][0]) for r in resid] == [0, 1, 2, 3, 1, 2, 0, 0]

    return out + [Case("age counts up and resets on a change of state", _cfg(64), steps, ages)]


def _other() -> List[Case]:
    rng = np.random.default_rng(5)
    q = Q0 + 2000

    def mixed(qh, C):
        n = 40
        g = rng.integers(0, C + 1, n)
        start = (qh - rng.integers(1, 12, n)) * BIN + rng.integers(0, BIN, n)
        return reqs(g, start, rng.integers(0, 8, n) * 0.125)

    groups = [3, 1, 0, 2, 4, 4]
    changing = Case("n_groups changing", _cfg(64, group_cap=4), [(mixed(q + 5 * w, 4), cut_of(q + 5 * w), G)
                                                                 for w, G in enumerate(groups)])

    steps = [(EMPTY, cut_of(q), 2)]
    for w in range(1, 9):  # windows of 4 bins; service 1 stops after the fourth
        lo, hi = q + 4 * (w - 1), q + 4 * w - 1
        steps.append((cat(traffic(0, lo, hi, 3, 0.25), traffic(1, lo, hi, 3, 0.25) if w <= 4 else EMPTY), cut_of(hi + 1), 2))

    def silent(res, resid):
        s0 = [int(r["rows"]["state"][0]) for r in res]
        s1 = [int(r["rows"]["state"][1]) for r in res]
        assert s0[-4:] == [0, 0, 0, 0] and 3 in s1 and s1[:4] == [4, 4, 4, 4], (s0, s1)
        assert int(res[-1]["rows"]["arr_recent"][1]) == 0 and int(res[-1]["rows"]["arr_base"][1]) > 0

    a = traffic(0, q - 8, q - 1, 16, 0.25)  # 128 spans
    assert len(a) == 128
    bound = Case("refused at ring_records_max", _cfg(64, ring_records_max=300),
                 [(a, cut_of(q), 1), (a, cut_of(q + 8), 1), (a, cut_of(q + 16), 1), (a[:44], cut_of(q + 16), 1),
                  (a[:45], cut_of(q + 63), 1), (a, cut_of(q + 64), 1)], refused=(2, 4))
    return [changing, Case("a service going silent", _cfg(64), steps, silent), bound]


def _random(name: str, B: int, C: int, seed: int, n_steps: int, n_max: int, span_cap: int = 512) -> Case:
    """Random multi-step runs with every placement case: durations up to a few bins and, rarely, longer
    than the ring; late, clipped, too old and future records; standing, jumping and backward cuts."""
    rng = np.random.default_rng(seed)
    steps, q_hi = [], Q0 + 5000
    for w in range(n_steps):
        move = int(rng.choice([0, 1, 3, 9, B // 2, B + 3], p=[0.15, 0.3, 0.25, 0.2, 0.07, 0.03]))
        cut_q = q_hi + move if rng.random() > 0.1 else q_hi - 2
        q_hi = max(q_hi, cut_q)
        n = int(rng.integers(0, n_max + 1))
        dur_us = np.where(rng.random(n) < 0.1, rng.integers(0, 2 * B * BIN, n), rng.integers(0, 6 * BIN, n))
        end = (q_hi + 1) * BIN - 1 - rng.integers(0, 20 * BIN, n) + np.where(rng.random(n) < 0.05, 30 * BIN, 0)
        end = np.where(rng.random(n) < 0.05, end - B * BIN, end)
        r = reqs(rng.integers(0, C + 1, n), end - dur_us, dur_us / 1000.0)
        r["flags"] = np.where(rng.random(n) < 0.1, R.SPAN_FIRST_TOKEN, np.where(rng.random(n) < 0.3, R.SPAN_NO_SLI, 0))
        if n > 3:
            r["latency_ms"][0], r["ts_ns"][1], r["latency_ms"][2] = np.nan, 0, -3.0
        steps.append((r, cut_of(cut_q), int(rng.integers(0, C + 1))))
    return Case(name, _cfg(B, group_cap=C, span_cap=span_cap, min_requests=3), steps)


def _hot() -> List[Case]:
    qh = Q0 + 9000

    def total(n):
        def check(res, resid):
            assert int(res[-1]["rows"]["arr_ring"].sum()) == n == _stat(res[-1], "observed")
        return check

    one_key = reqs([1] * 250, [(qh - 3) * BIN + i for i in range(250)], [0.5] * 250)
    # 256 records of one workgroup, each with a start key and an end key of its own: 512 keys for 256 slots
    B = 128
    i = np.arange(256)
    wide = reqs(i % 4, (qh - B + 1 + (i // 4) * 2) * BIN + 700, [1.0] * 256)
    two_groups = reqs([0] * 512, [(qh - 4) * BIN + i for i in range(512)], [1.5] * 512)
    return [Case("hot one key", _cfg(64), [(one_key, cut_of(qh), 2)], total(250)),
            Case("hot more keys than LDS slots", _cfg(B, group_cap=4), [(wide, cut_of(qh), 4)], total(256)),
            Case("hot second workgroup's flush", _cfg(64, span_cap=512), [(two_groups, cut_of(qh), 1)], total(512)),
            _random("hot random", 128, 4, 77, 12, 500)]


def cases() -> List[Case]:
    return (_geometry() + _placement() + _advance() + _ring() + _states() + _compares() + _other() +
            [_random("random B=64", 64, 3, 3, 14, 120, span_cap=256)] + _hot())


CASE_NAMES = [c.name for c in cases()]
assert len(set(CASE_NAMES)) == len(CASE_NAMES)


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


def run_pipeline(engine: str, windows: List[np.ndarray], cuts: Sequence[int], n_groups, bins: int, group_cap: int = 8,
                 **kw):
    """The windows through ``WindowPipeline(engine, load_sli=bins)`` and a ``RingWindowSource`` over a
    span ring, cut at ``cuts`` (0: a cut without a time). Returns (per-window results, per-window
    tracker results (empty with ``bins`` = 0), windows the tracker skipped)."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import Cut, RingWindowSource, WindowPipeline
    from llm_slo_ebpf_toolkit_amd.runtime import load

    rt = load()
    if bins:
        kw = dict(dict(load_bin_us=BIN, load_settle_bins=SETTLE, load_recent_bins=RECENT, load_min_base_bins=MIN_BASE,
                       load_min_requests=4, load_min_conc_milli=500), **kw)
    pipe = WindowPipeline(4096, 1024, group_cap, model="bayes", learn=False, user_cap=1024, engine=engine,
                          ttft_slo_ms=800.0, window_ms=16.0, load_sli=bins, **kw)
    ring = rt.HostRing(1 << 12, 64)
    src = RingWindowSource(pipe, None, None, ring)
    res, loads = [], []
    try:
        for w, recs in enumerate(windows):
            G = n_groups if np.isscalar(n_groups) else n_groups[w]
            assert ring.push(recs) == len(recs)
            kk = src.stage(Cut(kernel=0, user=0, spans=ring.head, t_ns=int(cuts[w])), G)["k"]
            res.append({key: np.array(v, copy=True) for key, v in pipe.results(kk, G).items()})
            if bins:
                loads.append({key: np.array(v, copy=True) for key, v in pipe.load_results(kk, G).items()})
        src.drain()
        skipped = pipe.load_skipped
    finally:
        pipe.close()
    return res, loads, skipped
