"""Span windows for the saturation curve tests (pipeline/satcurve.py, ops/satcurve.py): builders of
finishing records with a start, a duration and a TTFT, the named cases both test files run (CASES), and
the brute force the oracle is checked against -- every request kept as its interval, every bin's busy time,
level and share of the curve computed from the intervals themselves (no cells, no idle time, no carry, no
prefix sums, no generations: folded bins are kept by their exact epoch), and the knee found by trying
every level directly."""

from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.pipeline import satcurve as sat
from llm_slo_ebpf_toolkit_amd.pipeline.decodesli import bucket_of

F32 = np.float32
BIN = 1000                              # 1 ms bins, in microseconds
B = 64
T0_US = 1_700_000_000_000_000           # a bin edge and an epoch edge: T0_US // BIN % 128 == 0
Q0 = T0_US // BIN
assert Q0 % 128 == 0
SETTLE, RECENT = 2, 4
SLO = 800.0
OK, BREACH = 100.0, 900.0               # TTFTs below and above the SLO
DAY_MS = 86_400_000.0
NOT_AN_END = R.SPAN_START | R.SPAN_FIRST_TOKEN
K, NONE = sat.K, sat.NONE


def reqs(grp: Sequence[int], start_us: Sequence[int], dur_ms, ttft_ms=OK, flags=0, ns: int = 0) -> np.ndarray:
    """Finishing records: service, start in microseconds (``ns`` more nanoseconds), duration and TTFT in ms."""
    n = len(grp)
    r = np.zeros(n, dtype=R.SPAN)
    r["group_id"] = np.asarray(grp, dtype=np.uint32)
    r["ts_ns"] = np.asarray(start_us, dtype=np.int64) * 1000 + ns
    r["latency_ms"] = np.broadcast_to(np.asarray(dur_ms, dtype=F32), (n,))
    r["ttft_ms"] = np.broadcast_to(np.asarray(ttft_ms, dtype=F32), (n,))
    r["flags"] = flags
    r["trace_h"] = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    return r


def req(g: int, q: int, off_us: int, dur_ms: float, ttft_ms: float = OK, flags=0, ns: int = 0) -> np.ndarray:
    """One request of service g starting ``off_us`` into bin q."""
    return reqs([g], [q * BIN + off_us], [dur_ms], [ttft_ms], flags, ns)


def cat(*parts: np.ndarray) -> np.ndarray:
    return np.concatenate(parts) if parts else np.zeros(0, R.SPAN)


EMPTY = np.zeros(0, R.SPAN)


def full(g: int, q: int, k: int, breaches: int = 0, bins: int = 1) -> np.ndarray:
    """``k`` requests of service g that fill each of the ``bins`` bins from q exactly (start on its edge, one
    bin long): the bin's busy time is k bins, its level ``bucket_of(8 k)``; the first ``breaches`` of every
    bin are above the SLO. A request ends on the next bin's edge and adds no busy time there."""
    qs = np.repeat(np.arange(q, q + bins, dtype=np.int64), k)
    ttft = np.tile(np.where(np.arange(k) < breaches, BREACH, OK), bins)
    return reqs([g] * len(qs), qs * BIN, 1.0, ttft)


def level_of_k(k: int) -> int:
    return int(bucket_of(min(8 * k, sat.MAX_U)))


def traffic(g: int, q_from: int, q_to: int, per_bin: int, dur_ms: float, ttft_ms: float = OK) -> np.ndarray:
    """``per_bin`` requests of service g in every bin of [q_from, q_to], evenly spaced from the bin's edge."""
    qs = np.repeat(np.arange(q_from, q_to + 1, dtype=np.int64), per_bin)
    off = np.tile(np.arange(per_bin, dtype=np.int64) * (BIN // max(per_bin, 1)), q_to - q_from + 1)
    return reqs([g] * len(qs), qs * BIN + off, dur_ms, ttft_ms)


def cut_of(q: int) -> int:
    """A cut inside bin q, ns."""
    return (q * BIN + BIN // 2) * 1000


# ---- the brute force ----------------------------------------------------------------------------
class Brute:
    """The rules request by request. Every placed request is kept as (service, ts_us, te_us, qe, the bin its
    start was placed in or -1, has a TTFT, breach). A bin's busy time is the sum of the overlaps of the
    intervals with it; its share of the curve the requests whose start was placed in it. A bin that leaves
    the ring is computed once more, from what is known then, and kept under its exact epoch."""

    def __init__(self, bins, bin_us, settle_bins, recent_bins, epoch_bins, budget_ppm, min_requests, slo_ms, group_cap,
                 **_kw):
        self.B, self.bin, self.C = bins, bin_us, group_cap
        self.settle, self.R, self.epoch = settle_bins, recent_bins, epoch_bins
        self.budget, self.min_requests, self.slo = budget_ppm, min_requests, F32(slo_ms)
        self.reqs: List[Tuple[int, int, int, int, int, bool, bool]] = []
        self.folded: Dict[int, np.ndarray] = {}  # epoch -> [C, K, 2]
        self.q_hi = self.q_first = -1
        self.age = [0] * group_cap

    def bins_of(self, g: int, q_lo: int, count: int):
        """(busy, n, b) of service g per bin of [q_lo, q_lo + count), from the intervals."""
        mine = np.array([(ts, te, qe, qs, has, br) for s, ts, te, qe, qs, has, br in self.reqs if s == g],
                        np.int64).reshape(-1, 6)
        ts, te, qs = mine[:, 0][:, None], mine[:, 1][:, None], mine[:, 3][:, None]
        has, br = mine[:, 4][:, None] != 0, mine[:, 5][:, None] != 0
        t = (q_lo + np.arange(count, dtype=np.int64))[None, :]
        lo = t * self.bin
        busy = np.clip(np.minimum(te, lo + self.bin) - np.maximum(ts, lo), 0, None).sum(axis=0)
        n = ((qs == t) & has).sum(axis=0)
        b = ((qs == t) & has & br).sum(axis=0)
        return busy, n, b

    def levels(self, busy):
        return [int(bucket_of(min(int(x) * 8 // self.bin, sat.MAX_U))) for x in busy]

    def step(self, recs: np.ndarray, cut_ns: int, n_groups: int) -> Dict[str, np.ndarray]:
        prev, Bn, bin_us = self.q_hi, self.B, self.bin
        self.q_hi = q_hi = max(self.q_hi, (cut_ns // 1000) // bin_us)
        if prev != -1 and q_hi > prev:  # the bins that leave the ring, from what is known now
            first = prev - Bn + 1
            count = min(Bn, q_hi - prev)
            for g in range(self.C):
                busy, n, b = self.bins_of(g, first, count)
                for j, level in enumerate(self.levels(busy)):
                    e = first + j
                    if e >= self.q_first and n[j]:
                        gen = self.folded.setdefault(e // self.epoch, np.zeros((self.C, K, 2), np.uint64))
                        gen[g, level] += np.array([n[j], b[j]], np.uint64)
        if prev == -1 or q_hi - prev >= Bn:
            self.q_first = q_hi
        oldest = q_hi - Bn + 1
        stats = dict.fromkeys(sat.STATS, 0)
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
            ttft = F32(r["ttft_ms"])
            has = bool(ttft >= F32(0))
            if not has:
                stats["no_ttft"] += 1
            ts = ts_ns // 1000
            te = ts + int(float(v) * 1000.0)  # a Python float is an IEEE double; int() truncates
            qe = te // bin_us
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
            qs = ts // bin_us
            if qs < oldest:
                stats["clipped"] += 1
                qs = -1
            self.reqs.append((g, ts, te, qe, qs, has, bool(has and ttft > self.slo)))
        st = np.array([stats[name] for name in sat.STATS], np.uint32)
        rows, curve = self.rows()
        return {"rows": rows, "curve": curve, "stats": st}

    def knee(self, curve) -> Tuple[int, int, int]:
        """(level or NONE, n, b): every level tried directly."""
        d = [int(curve[l][1]) * 1_000_000 - self.budget * int(curve[l][0]) for l in range(K)]
        S = [sum(d[l:]) for l in range(K)]
        top = max(S)
        if top <= 0:
            return NONE, 0, 0
        level = max(l for l in range(K) if S[l] == top)
        return level, sum(int(curve[j][0]) for j in range(level, K)), sum(int(curve[j][1]) for j in range(level, K))

    def rows(self):
        out = sat.unknown_rows(self.C)
        curve = np.zeros((self.C, K, 2), np.uint64)
        q_hi, oldest = self.q_hi, self.q_hi - self.B + 1
        lo = max(oldest, self.q_first)
        hi = q_hi - self.settle
        rec_lo = hi - self.R + 1
        x_now = max(oldest - 1, 0) // self.epoch
        for x in (x_now, x_now - 1):
            if x in self.folded:
                curve += self.folded[x]
        for g in range(self.C):
            busy, n, b = self.bins_of(g, oldest, self.B)
            for j, level in enumerate(self.levels(busy)):
                if lo <= oldest + j <= hi:
                    curve[g, level] += np.array([n[j], b[j]], np.uint64)
            row = out[g]
            n_total = int(curve[g, :, 0].sum())
            row["n_total"], row["b_total"] = n_total, int(curve[g, :, 1].sum())
            have = [l for l in range(K) if curve[g, l, 0]]
            if have:
                row["top_level"] = have[-1]
            level, kn, kb = self.knee(curve[g])
            valid = level != NONE and kn >= self.min_requests
            state = sat.UNKNOWN
            if rec_lo >= lo and n_total >= self.min_requests:
                busy_recent = int(busy[rec_lo - oldest:hi - oldest + 1].sum())
                recent_u = min(busy_recent * 8 // (self.R * self.bin), sat.MAX_U)
                row["busy_recent"], row["recent_u"] = busy_recent, recent_u
                state = sat.NO_KNEE
                if valid:
                    row["knee_level"], row["n_knee"], row["b_knee"] = level, kn, kb
                    state = sat.BELOW if int(bucket_of(recent_u)) < level else sat.SATURATED
            self.age[g] = min(self.age[g] + 1, 2 ** 32 - 1) if state == sat.SATURATED else 0
            row["state"], row["age"] = state, self.age[g]
        return out, curve


def same_rows(a: np.ndarray, b: np.ndarray, what: str = "") -> None:
    """Rows compared as bytes."""
    assert a.dtype == b.dtype == sat.SAT_ROW and a.shape == b.shape, (what, a.dtype, a.shape, b.shape)
    if np.ascontiguousarray(a).tobytes() != np.ascontiguousarray(b).tobytes():
        raise AssertionError(f"{what}: rows differ\n{a}\n{b}")


def same_results(a: dict, b: dict, what: str = "") -> None:
    assert set(a) == set(b) == set(sat.RESULT_FIELDS), what
    same_rows(a["rows"], b["rows"], what)
    assert a["curve"].dtype == b["curve"].dtype == np.uint64 and a["curve"].shape == b["curve"].shape == \
        (len(a["rows"]), K, 2), (what, a["curve"].dtype, a["curve"].shape, b["curve"].shape)
    np.testing.assert_array_equal(a["curve"], b["curve"], err_msg=f"{what} curve")
    assert a["stats"].dtype == b["stats"].dtype == np.uint32 and a["stats"].shape == b["stats"].shape == (sat.N_STATS,)
    np.testing.assert_array_equal(a["stats"], b["stats"], err_msg=f"{what} stats")


RESIDENT = (("counts", np.uint64), ("idle_us", np.uint64), ("sli", np.uint64), ("carry", np.int32), ("gen", np.uint64),
            ("age", np.uint32))


def same_resident(a: dict, b: dict, what: str = "") -> None:
    assert (int(a["q_hi"]), int(a["q_first"])) == (int(b["q_hi"]), int(b["q_first"])), (what, a["q_hi"], b["q_hi"])
    assert tuple(a["gen_epoch"]) == tuple(b["gen_epoch"]), (what, a["gen_epoch"], b["gen_epoch"])
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
    refused: Dict[int, str] = {}                      # steps that must be refused, changing nothing: the message


def _cfg(group_cap=3, span_cap=256, epoch_bins=64, budget_ppm=100_000, min_requests=4, **kw):
    return dict(bins=B, bin_us=BIN, settle_bins=SETTLE, recent_bins=RECENT, epoch_bins=epoch_bins, budget_ppm=budget_ppm,
                min_requests=min_requests, slo_ms=SLO, group_cap=group_cap, span_cap=span_cap, **kw)


def _stat(res, name):
    return int(res["stats"][sat.STATS.index(name)])


# One step that sets q_first = QF, one at QF + 13 with the records: the curve's ring part is the 12 bins
# QF .. QF + 11, the recent range QF + 8 .. QF + 11, the last two bins settle.
QF = Q0 + 1024
CUT = QF + 13
REC = QF + 8


def _two(name, recs, check, G=3, **kw) -> Case:
    return Case(name, _cfg(**kw), [(EMPTY, cut_of(QF), G), (recs, cut_of(CUT), G)], check)


def _curve_is(g, want: Dict[int, Tuple[int, int]], extra=None):
    """The last step's curve of service g: {level: (n, b)}, every other level empty."""
    def check(res, resid):
        c = res[-1]["curve"][g]
        got = {int(l): (int(c[l, 0]), int(c[l, 1])) for l in np.nonzero(c[:, 0] | c[:, 1])[0]}
        assert got == want, got
        row = res[-1]["rows"][g]
        assert (int(row["n_total"]), int(row["b_total"])) == (sum(v[0] for v in want.values()), sum(v[1] for v in want.values()))
        assert int(row["top_level"]) == (max(want) if want else NONE)
        if extra is not None:
            extra(res, resid)
    return check


def _geometry() -> List[Case]:
    q = QF + 3
    return [_two("inside one bin", req(1, q, 100, 0.5, ns=999), _curve_is(1, {4: (1, 0)})),        # busy 500: u = 4
            _two("across three bins", req(1, q, 600, 2.0, BREACH), _curve_is(1, {3: (1, 1)})),      # 400 in its bin: u = 3
            _two("ending on a bin's edge", req(1, q, 500, 0.5), _curve_is(1, {4: (1, 0)})),
            _two("zero duration", req(1, q, 250, 0.0), _curve_is(1, {0: (1, 0)})),
            # the spanning request lifts the next bin's level: 100 + 125 us there
            _two("two in a bin, one spanning", cat(req(1, q, 0, 0.25), req(1, q, 900, 0.2), req(1, q + 1, 10, 0.125, BREACH)),
                 _curve_is(1, {2: (2, 0), 1: (1, 1)}))]


def _placement() -> List[Case]:
    oldest = CUT - 63

    def stats_are(sli_sum=None, **want):
        def check(res, resid):
            got = sat.stats_dict(res[-1]["stats"])
            assert got == dict(dict.fromkeys(sat.STATS, 0), **want), got
            if sli_sum is not None:
                assert int(resid[-1]["sli"].sum()) == sli_sum, resid[-1]["sli"].sum()
        return check

    def clipped(res, resid):
        stats_are(0, observed=1, clipped=1)(res, resid)
        assert int(resid[-1]["carry"][0]) == 1 and int(res[-1]["rows"]["n_total"][0]) == 0

    def future_start(res, resid):
        stats_are((1 << 32) | 1, observed=1, future=1)(res, resid)
        assert int(resid[-1]["sli"][0, CUT & 63]) == (1 << 32) | 1 and int(resid[-1]["idle_us"][0, CUT & 63]) == BIN

    above_a_day = float(np.nextafter(F32(DAY_MS), F32(np.inf)))
    flags_that_do_not_matter = R.SPAN_NO_SLI | R.SPAN_LATE | R.pack_outcome(5) | R.pack_tpot_us(1234)
    at = (CUT - 9) * BIN
    return [
        _two("clipped", req(0, oldest - 7, 500, 10.0, BREACH), clipped),
        _two("clipped without a ttft", req(0, oldest - 7, 500, 10.0, np.nan), stats_are(0, observed=1, clipped=1, no_ttft=1)),
        _two("too old", cat(req(0, oldest - 7, 500, 6.0), req(0, oldest - 1, 0, 0.999, -1.0)),
             stats_are(0, observed=2, too_old=2, no_ttft=1)),
        _two("a future start", req(0, CUT + 3, 10, 1.0, BREACH), future_start),
        _two("a future start without a ttft", req(0, CUT + 3, 10, 1.0, np.nan), stats_are(0, observed=1, future=1, no_ttft=1)),
        _two("a future end", req(0, CUT - 1, 300, 5.0), stats_are(1, observed=1, future=1)),
        _two("no time", cat(reqs([0, 1], [0, -5], 1.0), req(2, CUT - 9, 0, 0.5, np.nan)),
             stats_are(0, observed=1, no_time=2, no_ttft=1)),
        _two("invalid latencies", reqs([0] * 6, [at] * 6, [np.nan, -1.0, np.inf, above_a_day, -np.inf, -0.0]),
             stats_are(1, observed=1, invalid=5)),
        _two("out of group", reqs([2, 3, 700, 1], [at] * 4, 0.5), stats_are(1, observed=1, out_of_group=3), G=2),
        _two("start and first-token records skipped",
             cat(req(0, CUT - 9, 0, 0.5, OK, R.SPAN_START | R.SPAN_NO_SLI), req(0, CUT - 9, 0, 0.5, OK, R.SPAN_FIRST_TOKEN),
                 req(7, CUT - 9, 0, np.nan, OK, R.SPAN_FIRST_TOKEN | R.SPAN_LATE), req(1, CUT - 9, 0, 0.5)),
             stats_are(1, observed=1)),
        _two("a no-sli finishing record carries its ttft", req(0, CUT - 9, 0, 0.5, BREACH, flags_that_do_not_matter),
             stats_are((1 << 32) | 1, observed=1)),
        # -0.0 >= 0 holds: a TTFT; the SLO itself is no breach, the next float32 above it is one
        _two("ttft validity and the breach compare",
             reqs([0] * 7, [at] * 7, 0.5, [np.nan, -1.0, -np.inf, -0.0, SLO, float(np.nextafter(F32(SLO), F32(np.inf))), np.inf]),
             stats_are((2 << 32) | 4, observed=7, no_ttft=3)),
        # a fast failure without a TTFT still loads the service: it lifts the level of the bin a request with one is in
        _two("a request without a ttft occupies its interval", cat(full(0, QF + 3, 1), reqs([0] * 3, [(QF + 3) * BIN] * 3, 1.0, np.nan)),
             _curve_is(0, {level_of_k(4): (1, 0)}, stats_are(1, observed=4, no_ttft=3))),
    ]


def _levels() -> List[Case]:
    q = QF + 3

    def lv(name, k, tail_us, want_u):
        """k requests that fill bin q and one that is in it for its last ``tail_us`` microseconds."""
        recs = cat(full(0, q, k), req(0, q, BIN - tail_us, tail_us / 1000.0) if tail_us else EMPTY)
        n = k + (1 if tail_us else 0)
        assert min((k * BIN + tail_us) * 8 // BIN, sat.MAX_U) == want_u
        return _two(name, recs, _curve_is(0, {int(bucket_of(want_u)): (n, 0)}), span_cap=2048, min_requests=1)

    return [lv("level at u = 15", 1, 875, 15), lv("level at u = 16", 2, 0, 16), lv("level at u = 17", 2, 125, 17),
            lv("level at u = 8190", 1023, 750, 8190), lv("level at u = 8191", 1023, 875, 8191),
            lv("level above u = 8191", 1100, 0, 8191)]


def _advance() -> List[Case]:
    q = Q0 + 2048

    def win(qh, g=0):
        return cat(traffic(g, qh - 6, qh - 3, 2, 0.25), req(1, qh - 4, 100, 1.5, BREACH))

    def moves(expect):
        def check(res, resid):
            assert [(r["q_hi"], r["q_first"]) for r in resid] == expect
        return check

    several = [(win(q), cut_of(q), 2), (win(q), cut_of(q), 2), (win(q + 1), cut_of(q + 1), 2), (win(q + 6), cut_of(q + 6), 2)]
    back = [(win(q + 10), cut_of(q + 10), 2), (win(q + 3), cut_of(q + 3), 2), (EMPTY, 1000, 2), (win(q + 11), cut_of(q + 11), 2)]
    jump = [(EMPTY, cut_of(q), 2), (traffic(0, q, q + 18, 2, 0.25), cut_of(q + 20), 2),
            (win(q + 20 + B), cut_of(q + 20 + B), 2), (win(q + 21 + B), cut_of(q + 21 + B), 2),
            (win(q + 400), cut_of(q + 400), 2)]

    def jumped(res, resid):
        moves([(q, q), (q + 20, q), (q + 20 + B, q + 20 + B), (q + 21 + B, q + 20 + B), (q + 400, q + 400)])(res, resid)
        assert all(int(r["carry"].sum()) == 0 for r in resid)
        # the jump of exactly B folded the whole ring: 38 requests in the generations, the ring empty
        assert int(resid[2]["gen"][:, 0, :, 0].sum()) == 38 and int(res[2]["rows"]["n_total"][0]) == 38
        assert int(resid[2]["counts"].sum()) == int(resid[2]["counts"][:, (q + 20 + B - np.arange(7)) & 63].sum())

    return [Case("advance by 0, 1 and several bins", _cfg(), several, moves([(q, q), (q, q), (q + 1, q), (q + 6, q)])),
            Case("a cut moving back", _cfg(), back, moves([(q + 10, q + 10)] * 3 + [(q + 11, q + 10)])),
            Case("advance by B or more", _cfg(), jump, jumped)]


def _fold() -> List[Case]:
    q = QF

    # bins q - 1 (before q_first: no whole history) and q (exactly q_first), both leaving the ring in one advance
    def at_q_first(res, resid):
        assert int(res[1]["rows"]["n_total"][0]) == 3  # only bin q is in the curve while in the ring
        gen = resid[2]["gen"]
        assert int(gen[:, 0, :, 0].sum()) == 3 and int(gen[:, 0, :, 1].sum()) == 3 and int(gen[:, 1:].sum()) == 0
        assert int(res[2]["rows"]["n_total"][0]) == 3 and int(resid[2]["sli"].sum()) == 0

    first = Case("folded exactly at q_first and one bin before it", _cfg(epoch_bins=128),
                 [(EMPTY, cut_of(q), 1), (cat(full(0, q - 1, 2), full(0, q, 3, 3)), cut_of(q + 5), 1), (EMPTY, cut_of(q + 64), 1)],
                 at_q_first)

    # one request alone in bin q + 3 (level of u = 4); a late record that was in flight over the whole bin lifts it
    def late(res, resid):
        _curve_is(0, {4: (1, 0)})(res[:2], resid[:2])
        _curve_is(0, {int(bucket_of(12)): (1, 0), int(bucket_of(6)): (1, 1)})(res, resid)

    lifted = Case("a late record changes an unevicted bin's level", _cfg(),
                  [(EMPTY, cut_of(q), 1), (req(0, q + 3, 100, 0.5), cut_of(q + 13), 1),
                   (req(0, q + 2, 250, 2.0, BREACH), cut_of(q + 14), 1)], late)

    # the late record's start bin has left the ring: clipped, in carry, not in the curve
    def evicted(res, resid):
        assert _stat(res[2], "clipped") == 1 and int(resid[2]["carry"][0]) == 1
        assert [int(r["rows"]["n_total"][0]) for r in res] == [0, 2, 2]
        # it was in flight over the ring's oldest bins all the same: the bin of the second request is busier
        assert int(res[2]["curve"][0, int(bucket_of(8 + 2)), 0]) == 1

    gone = Case("a late record whose start bin is evicted", _cfg(epoch_bins=128),
                [(EMPTY, cut_of(q), 1), (cat(req(0, q + 2, 0, 0.25), req(0, q + 40, 0, 0.25)), cut_of(q + 45), 1),
                 (req(0, q + 20, 500, 20.75, BREACH), cut_of(q + 90), 1)], evicted)

    # bins q + 50 .. q + 80 hold 2 requests each; the advance to q + 146 evicts q + 20 .. q + 82: both epochs
    def crossed(res, resid):
        x = q // 64
        assert x % 2 == 0 and q % 64 == 0
        assert [r["gen_epoch"] for r in resid] == [(-1, -1), (-1, -1), (x, -1), (x, x + 1), (x + 2, x + 1), (x + 2, x + 3)]
        gen = resid[3]["gen"]
        assert int(gen[0, 0, :, 0].sum()) == 2 * 14 and int(gen[1, 0, :, 0].sum()) == 2 * 17
        # at q + 200 epoch x is two epochs old: its generation is gone, the one of x + 1 is still read
        assert [int(r["rows"]["n_total"][0]) for r in res] == [0, 0, 62, 62, 34, 0]
        assert int(resid[4]["gen"][0].sum()) == 0 and int(resid[5]["gen"].sum()) == 0

    epochs = Case("an epoch boundary crossed inside one advance, a generation dropped after two epochs", _cfg(),
                  [(EMPTY, cut_of(q), 1), (EMPTY, cut_of(q + 40), 1), (traffic(0, q + 50, q + 80, 2, 0.25), cut_of(q + 83), 1),
                   (EMPTY, cut_of(q + 146), 1), (EMPTY, cut_of(q + 200), 1), (EMPTY, cut_of(q + 64 * 4 + 20), 1)], crossed)

    def far(res, resid):
        assert [int(r["rows"]["n_total"][0]) for r in res] == [0, 10, 0, 10]
        assert int(resid[2]["gen"].sum()) == 10 + 0 and resid[2]["q_first"] == q + 64 * 5  # folded, but no longer read
        assert [int(r["rows"]["state"][0]) for r in res] == [0, 1, 0, 1]

    jump = Case("a jump over more than two epochs", _cfg(),
                [(EMPTY, cut_of(q), 1), (full(0, q + 3, 5, 0, 2), cut_of(q + 13), 1), (EMPTY, cut_of(q + 64 * 5), 1),
                 (full(0, q + 64 * 5 + 1, 5, 0, 2), cut_of(q + 64 * 5 + 6), 1)], far)
    return [first, lifted, gone, epochs, jump]


def _knee() -> List[Case]:
    def knee_is(level, n=0, b=0, state=None):
        def check(res, resid):
            row = res[-1]["rows"][0]
            assert (int(row["knee_level"]), int(row["n_knee"]), int(row["b_knee"])) == (level, n, b), row
            if state is not None:
                assert int(row["state"]) == state, row
        return check

    L8 = level_of_k(8)
    # budget 10 %: d = 10^5 (10 b - n)
    step_curve = cat(full(0, QF, 2, 0, 3), full(0, QF + 3, 4, 0, 2), full(0, QF + 5, 8, 4, 2))
    noisy = cat(full(0, QF, 1, 1, 3), full(0, QF + 3, 4, 0, 3), full(0, QF + 6, 6, 0, 3), full(0, QF + 9, 8, 2, 2))
    # S = 12 at the level of 8 (n 8, b 2) and again at the level of 2 (-4 from the level of 4, +4 from n 6, b 1)
    equal = cat(full(0, QF, 8, 2), full(0, QF + 1, 4), full(0, QF + 2, 2, 1), full(0, QF + 3, 2, 0, 2))
    zero = cat(full(0, QF, 5, 1), full(0, QF + 1, 5), full(0, QF + 2, 2, 0, 2))  # n 10, b 1 on top: d = 0
    at_min = cat(full(0, QF, 8, 8), full(0, QF + 1, 1, 0, 2))
    return [
        _two("knee of a clean step curve", step_curve, knee_is(L8, 16, 8, sat.BELOW)),
        _two("a noisy low level must not win", noisy, knee_is(L8, 16, 4)),
        _two("equal maxima: the larger level wins", equal, knee_is(L8, 8, 2)),
        _two("maximum exactly 0: no knee", zero, knee_is(NONE, state=sat.NO_KNEE)),
        _two("n_knee at min_requests", at_min, knee_is(L8, 8, 8), min_requests=8),
        _two("n_knee one below min_requests", at_min, knee_is(NONE, state=sat.NO_KNEE), min_requests=9),
        _two("budget compare at equality", full(0, QF, 10, 1), knee_is(NONE, state=sat.NO_KNEE)),
        _two("budget compare one above equality", full(0, QF, 10, 1), knee_is(level_of_k(10), 10, 1), budget_ppm=99_999),
    ]


def _states() -> List[Case]:
    q = QF
    curve = cat(full(0, q, 2, 0, 3), full(0, q + 3, 4, 0, 2), full(0, q + 8, 8, 4, 4))  # the recent bins are the busy ones

    def seq(want):
        def check(res, resid):
            got = [(int(r["rows"]["state"][0]), int(r["rows"]["age"][0])) for r in res]
            assert got == want, got
            assert [int(r["age"][0]) for r in resid] == [a for _, a in want]
        return check

    cut = cut_of(q + 13)
    # unknown; saturated on three standing cuts; the recent range moves on to an idle bin: below; a late record
    # fills that bin: saturated again, from 1; a jump: unknown (no_knee: the cases above)
    states = Case("the four states and age", _cfg(),
                  [(EMPTY, cut_of(q), 1), (curve, cut, 1), (EMPTY, cut, 1), (EMPTY, cut - 1, 1), (EMPTY, cut_of(q + 14), 1),
                   (full(0, q + 12, 8), cut_of(q + 14), 1), (EMPTY, cut_of(q + 100), 1)],
                  seq([(0, 0), (3, 1), (3, 2), (3, 3), (2, 0), (3, 1), (0, 0)]))

    def unknown_keeps(res, resid):
        row = res[-1]["rows"][0]
        assert int(row["state"]) == sat.UNKNOWN and int(row["n_total"]) == 3 and int(row["top_level"]) == level_of_k(3)
        assert (int(row["knee_level"]), int(row["n_knee"]), int(row["recent_u"]), int(row["busy_recent"])) == (NONE, 0, 0, 0)

    few = _two("unknown below min_requests keeps its totals", full(0, REC, 3, 3), unknown_keeps)

    def no_knee(res, resid):
        row = res[-1]["rows"][0]
        assert int(row["state"]) == sat.NO_KNEE and int(row["recent_u"]) == 8 * 6 // 4 and int(row["busy_recent"]) == 6 * BIN

    clean = _two("no knee inside the budget", full(0, REC, 3, 0, 2), no_knee)

    # age saturating is the host check's; two services with different states in one step
    def both(res, resid):
        assert [int(x) for x in res[-1]["rows"]["state"]] == [3, 1, 0]

    two = _two("services in different states", cat(curve, full(1, q + 2, 5, 0, 2)), both)
    return [states, few, clean, two]


def _other() -> List[Case]:
    rng = np.random.default_rng(5)
    q = Q0 + 4096

    def mixed(qh, C):
        n = 40
        g = rng.integers(0, C + 1, n)
        start = (qh - rng.integers(1, 12, n)) * BIN + rng.integers(0, BIN, n)
        return reqs(g, start, rng.integers(0, 8, n) * 0.125, np.where(rng.random(n) < 0.3, BREACH, OK))

    groups = [3, 1, 0, 2, 5, 5]
    changing = Case("n_groups changing", _cfg(group_cap=5), [(mixed(q + 5 * w, 5), cut_of(q + 5 * w), G)
                                                             for w, G in enumerate(groups)])
    a = traffic(0, q - 8, q - 1, 16, 0.25)  # 128 spans
    assert len(a) == 128
    ring = Case("refused at ring_records_max", _cfg(ring_records_max=300),
                [(a, cut_of(q), 1), (a, cut_of(q + 8), 1), (a, cut_of(q + 16), 1), (a[:44], cut_of(q + 16), 1),
                 (a[:45], cut_of(q + 63), 1), (a, cut_of(q + 64), 1)], refused={2: "ring_records_max", 4: "ring_records_max"})

    def at(w):
        return traffic(0, q + 64 * w - 8, q + 64 * w - 1, 16, 0.25)

    # 128 spans an epoch: the third epoch in a row would make 384; one epoch later the first has left the count
    curve = Case("refused at curve_records_max", _cfg(curve_records_max=300),
                 [(at(0), cut_of(q), 1), (at(1), cut_of(q + 64), 1), (at(2), cut_of(q + 128), 1), (at(2)[:44], cut_of(q + 128), 1),
                  (at(2)[:45], cut_of(q + 130), 1), (at(3), cut_of(q + 192), 1)],
                 refused={2: "curve_records_max", 4: "curve_records_max"})
    return [changing, ring, curve]


def _random(name: str, C: int, seed: int, n_steps: int, n_max: int, span_cap: int = 512, epoch_bins: int = 64) -> Case:
    """Random multi-step runs with every placement case: durations up to a few bins and, rarely, longer
    than the ring; late, clipped, too old and future records, with and without a TTFT; standing, jumping
    and backward cuts. The budget and min_requests are low enough for knees to appear and move."""
    rng = np.random.default_rng(seed)
    steps, q_hi = [], Q0 + 8192
    for w in range(n_steps):
        move = int(rng.choice([0, 1, 3, 9, B // 2, B + 3], p=[0.15, 0.3, 0.25, 0.2, 0.07, 0.03]))
        cut_q = q_hi + move if rng.random() > 0.1 else q_hi - 2
        q_hi = max(q_hi, cut_q)
        n = int(rng.integers(0, n_max + 1))
        dur_us = np.where(rng.random(n) < 0.1, rng.integers(0, 2 * B * BIN, n), rng.integers(0, 6 * BIN, n))
        end = (q_hi + 1) * BIN - 1 - rng.integers(0, 20 * BIN, n) + np.where(rng.random(n) < 0.05, 30 * BIN, 0)
        end = np.where(rng.random(n) < 0.05, end - B * BIN, end)
        ttft = np.where(rng.random(n) < 0.1, np.nan, np.where(rng.random(n) < 0.1 + 0.1 * (dur_us > 3 * BIN), BREACH, OK))
        r = reqs(rng.integers(0, C + 1, n), end - dur_us, dur_us / 1000.0, ttft)
        r["flags"] = np.where(rng.random(n) < 0.1, R.SPAN_FIRST_TOKEN, np.where(rng.random(n) < 0.3, R.SPAN_NO_SLI, 0))
        if n > 3:
            r["latency_ms"][0], r["ts_ns"][1], r["latency_ms"][2] = np.nan, 0, -3.0
        steps.append((r, cut_of(cut_q), int(rng.integers(0, C + 1))))
    return Case(name, _cfg(group_cap=C, span_cap=span_cap, min_requests=3, epoch_bins=epoch_bins, budget_ppm=150_000), steps)


def _hot() -> List[Case]:
    qh = QF + 13

    def total(n):
        def check(res, resid):
            assert int(res[-1]["rows"]["n_total"][1]) == n == _stat(res[-1], "observed")
            assert int(res[-1]["rows"]["b_total"][1]) == n // 4
        return check

    i = np.arange(4096)
    ttft = np.where(i % 4 == 0, BREACH, OK)
    one = reqs([1] * 4096, (QF + 3) * BIN + i % 500, 0.25, ttft)
    four = reqs([1] * 4096, (QF + 3 + i % 4) * BIN + (i // 4) % 500, 0.25, ttft)
    return [Case("hot one bin", _cfg(span_cap=4096), [(EMPTY, cut_of(QF), 2), (one, cut_of(qh), 2)], total(4096)),
            Case("hot four bins", _cfg(span_cap=4096), [(EMPTY, cut_of(QF), 2), (four, cut_of(qh), 2)], total(4096))]


def cases() -> List[Case]:
    return (_geometry() + _placement() + _levels() + _advance() + _fold() + _knee() + _states() + _other() +
            [_random("random epoch 64", 3, 3, 16, 120, span_cap=256), _random("random epoch 128", 5, 9, 12, 200, epoch_bins=128)] +
            _hot())


CASE_NAMES = [c.name for c in cases()]
assert len(set(CASE_NAMES)) == len(CASE_NAMES)


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


def run_pipeline(engine: str, windows: List[np.ndarray], cuts: Sequence[int], n_groups, bins: int, group_cap: int = 8,
                 **kw):
    """The windows through ``WindowPipeline(engine, saturation=bins)`` and a ``RingWindowSource`` over a
    span ring, cut at ``cuts`` (0: a cut without a time). Returns (per-window results, per-window
    tracker results (empty with ``bins`` = 0), windows the tracker skipped)."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import Cut, RingWindowSource, WindowPipeline
    from llm_slo_ebpf_toolkit_amd.runtime import load

    rt = load()
    if bins:
        kw = dict(dict(sat_bin_us=BIN, sat_settle_bins=SETTLE, sat_recent_bins=RECENT, sat_epoch_bins=64,
                       sat_budget_ppm=150_000, sat_min_requests=4), **kw)
    pipe = WindowPipeline(4096, 1024, group_cap, model="bayes", learn=False, user_cap=1024, engine=engine,
                          ttft_slo_ms=SLO, window_ms=16.0, saturation=bins, **kw)
    ring = rt.HostRing(1 << 12, 64)
    src = RingWindowSource(pipe, None, None, ring)
    res, sats = [], []
    try:
        for w, recs in enumerate(windows):
            G = n_groups if np.isscalar(n_groups) else n_groups[w]
            assert ring.push(recs) == len(recs)
            kk = src.stage(Cut(kernel=0, user=0, spans=ring.head, t_ns=int(cuts[w])), G)["k"]
            res.append({key: np.array(v, copy=True) for key, v in pipe.results(kk, G).items()})
            if bins:
                sats.append({key: np.array(v, copy=True) for key, v in pipe.saturation_results(kk, G).items()})
        src.drain()
        skipped = pipe.sat_skipped
    finally:
        pipe.close()
    return res, sats, skipped
