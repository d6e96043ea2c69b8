"""Span windows for the breach-onset tests (pipeline/onset.py, ops/onset.py): builders of timed windows
with the rule's edge values, the named cases both test files run (CASES), and the brute force the
oracle is checked against -- a plain Python loop over a dict of absolute bins and the sequential
recurrence, no ring, no slots, no numpy reductions."""

from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.pipeline import onset as on
from tests.slisketch_scenarios import spans

F32 = np.float32
SLO = 800.0
BIN = 10_000_000                       # 10 ms bins
T0 = 1_700_000_000_000_000_000         # a bin edge: T0 % BIN == 0
Q0 = T0 // BIN
PER_WINDOW = 16                        # bins a window spans
GOOD, BAD = 100.0, 900.0
# equal to the SLO (no breach), just above it and +inf (breaches), -0.0 (counted, no breach), NaN and -1 (invalid)
EDGE_TTFT = [F32(800.0), np.nextafter(F32(800), F32(np.inf)), F32(np.inf), F32(-0.0), F32(np.nan), F32(-1.0)]


def timed(ttft: Sequence[float], grp: Sequence[int], ts: Sequence[int], flags=R.SPAN_FIRST_TOKEN) -> np.ndarray:
    r = spans(ttft, grp, flags)
    r["ts_ns"] = np.asarray(ts, dtype=np.int64)
    return r


def at_bins(g: int, bins_ttft: Sequence[Tuple[int, float]], off: int = 3) -> np.ndarray:
    """One record per (absolute bin, ttft) of service g, ``off`` ns into the bin."""
    return timed([v for _, v in bins_ttft], [g] * len(bins_ttft), [q * BIN + off for q, _ in bins_ttft])


def cut_of(q: int) -> int:
    """A cut inside bin q."""
    return q * BIN + BIN // 2


def edge_window(rng, n: int, G: int, q_hi: int, B: int) -> np.ndarray:
    """About ``n`` log-normal records of ``G`` services over the window's 16 bins up to ``q_hi``, plus, per
    service: start times exactly on a bin edge and one below it, 0 and negative, the bins q_hi - B
    (dropped) and q_hi - B + 1 (kept), q_hi + 1 (clamped), every edge TTFT; SPAN_LATE on some, and what
    the rule skips (SPAN_NO_SLI, start records, groups at and above ``G``)."""
    ts = (q_hi - rng.integers(0, PER_WINDOW, n)) * BIN + rng.integers(0, BIN, n)
    parts = [timed(rng.lognormal(np.log(300.0), 1.5, n), rng.integers(0, max(G, 1), n), ts)]
    for g in range(G):
        q = q_hi - 2 - g
        stamps = [q * BIN, q * BIN - 1, 0, -5, (q_hi - B) * BIN + 7, (q_hi - B + 1) * BIN, (q_hi - B + 1) * BIN - 1,
                  (q_hi + 1) * BIN, (q_hi + 1) * BIN - 1, (q_hi + 40) * BIN + 1]
        e = timed([BAD, GOOD] * (len(stamps) // 2), [g] * len(stamps), stamps)
        e["flags"][::3] |= R.SPAN_LATE
        parts.append(e)
        parts.append(timed(EDGE_TTFT, [g] * len(EDGE_TTFT), [q_hi * BIN + 11 + i for i in range(len(EDGE_TTFT))]))
    parts.append(timed([BAD, GOOD], [G, G + 3], [q_hi * BIN + 1, q_hi * BIN + 2]))
    parts.append(timed([120.0, BAD], [0, 0], [q_hi * BIN + 5] * 2, R.SPAN_NO_SLI))
    parts.append(timed([np.nan], [0], [q_hi * BIN + 6], R.SPAN_START | R.SPAN_NO_SLI))
    out = np.concatenate(parts)
    return out[rng.permutation(len(out))]


# ---- the brute force ----------------------------------------------------------------------------
class Brute:
    """The rules record by record: ``bins[(g, q)] = [n, b]`` keyed by the absolute bin, dropped once the
    ring no longer covers it; rows by the recurrence over q_hi - B + 1 .. q_hi."""

    def __init__(self, bins: int, bin_ns: int, ref_ppm: int, alarm: int, group_cap: int, slo_ms: float = SLO, **_kw):
        self.B, self.bin_ns, self.ref, self.h, self.C = bins, bin_ns, ref_ppm, alarm * 1_000_000, group_cap
        self.slo = float(F32(slo_ms))
        self.bins: Dict[Tuple[int, int], List[int]] = {}
        self.q_hi = -1

    def step(self, recs: np.ndarray, cut_ns: int, n_groups: int) -> Dict[str, np.ndarray]:
        self.q_hi = max(self.q_hi, cut_ns // self.bin_ns)
        for key in [k for k in self.bins if k[1] <= self.q_hi - self.B]:
            del self.bins[key]
        stats = dict.fromkeys(on.STATS, 0)
        for r in recs:
            if int(r["flags"]) & R.SPAN_NO_SLI:
                continue
            g, v, ts = int(r["group_id"]), float(r["ttft_ms"]), int(r["ts_ns"])
            if g >= n_groups:
                stats["out_of_group"] += 1
                continue
            if not v >= 0.0:
                stats["invalid"] += 1
                continue
            stats["observed"] += 1
            if ts <= 0:
                stats["no_time"] += 1
                continue
            q = ts // self.bin_ns
            if q > self.q_hi:
                stats["future"] += 1
                q = self.q_hi
            if q <= self.q_hi - self.B:
                stats["too_old"] += 1
                continue
            cell = self.bins.setdefault((g, q), [0, 0])
            cell[0] += 1
            cell[1] += int(v > self.slo)
        st = np.zeros(on.N_STATS, np.uint32)
        st[:len(on.STATS)] = [stats[name] for name in on.STATS]
        return {"rows": self.rows(), "stats": st}

    def rows(self) -> np.ndarray:
        out = np.zeros(self.C, on.ONSET_ROW)
        for g in range(self.C):
            S, since = 0, None  # since: (onset_q, alarm_q, peak, n, b) of the open excursion
            n_ring = b_ring = 0
            zero_seen = False
            for q in range(self.q_hi - self.B + 1, self.q_hi + 1):
                n, b = self.bins.get((g, q), (0, 0))
                n_ring, b_ring = n_ring + n, b_ring + b
                S = max(0, S + b * 1_000_000 - n * self.ref)
                if S == 0:
                    since, zero_seen = None, True
                    continue
                if since is None:
                    since = [q, -1, 0, 0, 0]
                since[2] = max(since[2], S)
                since[3], since[4] = since[3] + n, since[4] + b
                if since[1] < 0 and S >= self.h:
                    since[1] = q
            row = out[g]
            row["n_ring"], row["b_ring"], row["onset_q"], row["alarm_q"] = n_ring, b_ring, -1, -1
            if since is not None:
                row["state"] = 2 if since[1] >= 0 else 1
                row["flags"] = 0 if zero_seen else 1
                row["onset_q"], row["alarm_q"], row["s_now"], row["s_peak"] = since[0], since[1], S, since[2]
                row["n_exc"], row["b_exc"] = since[3], since[4]
        return out

    def resident(self) -> Dict[str, np.ndarray]:
        n, b = np.zeros((self.C, self.B), np.uint32), np.zeros((self.C, self.B), np.uint32)
        for (g, q), (cn, cb) in self.bins.items():
            n[g, q % self.B], b[g, q % self.B] = cn, cb
        return {"n": n, "b": b, "q_hi": self.q_hi}


def same_rows(a: np.ndarray, b: np.ndarray, what: str = "") -> None:
    """Rows compared as bytes."""
    assert a.dtype == b.dtype == on.ONSET_ROW and a.shape == b.shape, (what, a.dtype, a.shape, b.shape)
    if np.ascontiguousarray(a).tobytes() != np.ascontiguousarray(b).tobytes():
        raise AssertionError(f"{what}: rows differ\n{a}\n{b}")


def same_results(a: dict, b: dict, what: str = "", G: Optional[int] = None) -> None:
    assert set(a) == set(b) == set(on.RESULT_FIELDS), what
    same_rows(a["rows"] if G is None else a["rows"][:G], b["rows"] if G is None else b["rows"][:G], what)
    assert a["stats"].dtype == b["stats"].dtype == np.uint32 and a["stats"].shape == b["stats"].shape == (on.N_STATS,)
    np.testing.assert_array_equal(a["stats"], b["stats"], err_msg=f"{what} stats")


def same_resident(a: dict, b: dict, what: str = "") -> None:
    assert int(a["q_hi"]) == int(b["q_hi"]), (what, a["q_hi"], b["q_hi"])
    for f in ("n", "b"):
        assert a[f].dtype == b[f].dtype == np.uint32 and a[f].shape == b[f].shape, (what, f)
        np.testing.assert_array_equal(a[f], b[f], err_msg=f"{what} resident {f}")


# ---- the named cases ----------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    cfg: dict                                         # bins, ref_ppm, alarm, group_cap (+ span_cap)
    steps: List[Tuple[np.ndarray, int, int]]          # (records, cut_ns, n_groups)
    check: Optional[Callable[[List[dict]], None]] = None  # over every step's results (all rows of group_cap)


def _cfg(bins, group_cap=3, ref_ppm=250_000, alarm=3, span_cap=1024):
    return dict(bins=bins, bin_ns=BIN, ref_ppm=ref_ppm, alarm=alarm, group_cap=group_cap, span_cap=span_cap, slo_ms=SLO)


def _edges(B: int) -> Case:
    rng = np.random.default_rng(B)
    G = 3
    steps = [(edge_window(rng, 40, G, Q0 + PER_WINDOW * (w + 1), B), cut_of(Q0 + PER_WINDOW * (w + 1)), G) for w in range(6)]

    def check(res):
        tot = np.sum([r["stats"].astype(np.int64) for r in res], axis=0)
        st = on.stats_dict(tot)
        # per window and service: 10 stamped records (2 without a time, 2 ahead of the cut, 2 too old), 4 valid edge TTFTs
        assert st["observed"] == 6 * (40 + G * 14) and st["invalid"] == 6 * G * 2 and st["out_of_group"] == 6 * 2
        assert st["no_time"] == 6 * G * 2 and st["future"] == 6 * G * 2 and st["too_old"] == 6 * G * 2

    return Case(f"edges B={B}", _cfg(B), steps, check)


def _zero_at(B: int, idx: int, name: str) -> Case:
    """The last zero of S on ring index ``idx``: a breach two bins before it (S = 750000), three good
    records on it (S = 0), a breach right after it; nothing later, so S stays above 0 to q_hi."""
    q_hi = Q0 + 1000
    q0 = q_hi - B + 1
    recs = at_bins(1, [(q0 + idx - 2, BAD), (q0 + idx, GOOD), (q0 + idx, GOOD), (q0 + idx, GOOD), (q0 + idx + 1, BAD)])

    def check(res):
        row = res[-1]["rows"][1]
        assert int(row["state"]) == 1 and int(row["onset_q"]) == q0 + idx + 1 and int(row["flags"]) == 0
        assert int(row["s_now"]) == 750_000 == int(row["s_peak"]) and (int(row["n_exc"]), int(row["b_exc"])) == (1, 1)
        assert (int(row["n_ring"]), int(row["b_ring"])) == (5, 2) and int(row["alarm_q"]) == -1

    return Case(name, _cfg(B), [(recs, cut_of(q_hi), 2)], check)


def _threshold(exact: bool) -> Case:
    """S reaches exactly h (ref 500000: two lone breaches, h = 1000000) or h - 1 (ref 1: one lone breach)."""
    q_hi = Q0 + 500
    recs = at_bins(0, [(q_hi - 9, BAD), (q_hi - 4, BAD)] if exact else [(q_hi - 4, BAD)])

    def check(res):
        row = res[-1]["rows"][0]
        if exact:
            assert int(row["s_now"]) == 1_000_000 and int(row["state"]) == 2 and int(row["alarm_q"]) == q_hi - 4
            assert int(row["onset_q"]) == q_hi - 9
        else:
            assert int(row["s_now"]) == 999_999 and int(row["state"]) == 1 and int(row["alarm_q"]) == -1

    return Case(f"threshold {'h' if exact else 'h - 1'}", _cfg(64, ref_ppm=500_000 if exact else 1, alarm=1),
                [(recs, cut_of(q_hi), 1)], check)


def _clipped() -> Case:
    q_hi, B = Q0 + 700, 64
    recs = at_bins(2, [(q_hi - B + 1, BAD), (q_hi - 30, BAD), (q_hi - 29, BAD), (q_hi - 28, BAD), (q_hi - 27, BAD), (q_hi, GOOD)])

    def check(res):
        row = res[-1]["rows"][2]
        assert int(row["flags"]) == 1 and int(row["onset_q"]) == q_hi - B + 1 and int(row["state"]) == 2
        assert int(row["alarm_q"]) == q_hi - 28 and int(row["s_peak"]) == 3_750_000 and int(row["s_now"]) == 3_500_000
        assert (int(row["n_exc"]), int(row["b_exc"])) == (6, 5)

    return Case("clipped", _cfg(B), [(recs, cut_of(q_hi), 3)], check)


def _quiet_after_peak() -> Case:
    q_hi = Q0 + 300
    recs = at_bins(0, [(q_hi - 20, BAD)] * 5 + [(q_hi, GOOD)] * 15)

    def check(res):
        row = res[-1]["rows"][0]
        assert int(row["state"]) == 0 and (int(row["onset_q"]), int(row["alarm_q"])) == (-1, -1)
        assert not int(row["s_now"]) and not int(row["s_peak"]) and not int(row["n_exc"]) and not int(row["b_exc"])
        assert (int(row["n_ring"]), int(row["b_ring"])) == (20, 5)

    return Case("quiet after a peak", _cfg(128), [(recs, cut_of(q_hi), 1)], check)


def _late_record() -> Case:
    q1 = Q0 + 400
    first = at_bins(0, [(q1, BAD), (q1, BAD)])
    late = at_bins(0, [(q1 - 5, BAD), (q1 + 20, GOOD)])
    late["flags"][0] |= R.SPAN_LATE

    def check(res):
        assert int(res[0]["rows"][0]["onset_q"]) == q1 and int(res[1]["rows"][0]["onset_q"]) == q1 - 5
        assert int(res[1]["rows"][0]["b_exc"]) == 3 and int(res[1]["rows"][0]["s_now"]) == 2_000_000

    return Case("late record", _cfg(64), [(first, cut_of(q1 + 2), 1), (late, cut_of(q1 + 2 + PER_WINDOW), 1)], check)


def _wrap() -> Case:
    rng = np.random.default_rng(9)
    B, G = 64, 3
    steps = []
    for w in range(10):  # 160 bins of time over a ring of 64
        q_hi = Q0 + PER_WINDOW * (w + 1)
        steps.append((edge_window(rng, 30, G, q_hi, B), cut_of(q_hi), G))
    return Case("ring wrap", _cfg(B), steps)


def _cuts() -> Case:
    """A jump of B bins and more, two steps on the same q_hi, a cut earlier than the one before."""
    rng = np.random.default_rng(10)
    B, G = 64, 2
    qs = [Q0 + 16, Q0 + 16, Q0 + 10, Q0 + 16 + B, Q0 + 16 + B + 3 * B + 5, Q0 + 16 + B + 3 * B + 5, Q0 + 16 + 5 * B]
    steps = []
    q_hi = -1
    for q in qs:
        q_hi = max(q_hi, q)
        steps.append((edge_window(rng, 25, G, q_hi, B), cut_of(q), G))

    def check(res):
        assert sum(int(r["rows"]["n_ring"].sum()) for r in res) > 100

    return Case("jumping and standing cuts", _cfg(B, group_cap=2), steps, check)


def _shapes() -> Case:
    rng = np.random.default_rng(11)
    B, C = 64, 4
    groups = [4, 0, 2, 3, 1, 4]
    steps = []
    for w, G in enumerate(groups):
        q_hi = Q0 + PER_WINDOW * (w + 1)
        recs = np.zeros(0, R.SPAN) if w == 2 else edge_window(rng, 30, max(G, 2), q_hi, B)
        steps.append((recs, cut_of(q_hi), G))
    return Case("empty step, no groups, changing groups", _cfg(B, group_cap=C), steps)


def _hot(spread: bool) -> Case:
    rng = np.random.default_rng(12)
    q_hi = Q0 + 2000
    v = rng.lognormal(np.log(600.0), 1.0, 4096).astype(F32)
    ts = (q_hi - (rng.integers(0, PER_WINDOW, 4096) if spread else 0)) * BIN + rng.integers(0, BIN, 4096)
    recs = timed(v, np.ones(4096, np.int64), ts)

    def check(res):
        row = res[-1]["rows"][1]
        assert int(row["n_ring"]) == 4096 and int(row["b_ring"]) == int((v > F32(SLO)).sum()) > 500

    return Case(f"hot {'16 bins' if spread else 'one bin'}", _cfg(1024, group_cap=2, ref_ppm=20_000, span_cap=4096),
                [(recs, cut_of(q_hi), 2)], check)


def _random() -> Case:
    rng = np.random.default_rng(13)
    B, C = 256, 5
    steps, q_hi = [], Q0
    for _ in range(20):
        q_hi += int(rng.integers(0, 40))
        G = int(rng.integers(0, C + 1))
        n = int(rng.integers(0, 200))
        ts = (q_hi - rng.integers(0, 60, n)) * BIN + rng.integers(0, BIN, n)
        v = np.where(rng.random(n) < 0.25, BAD, GOOD)
        steps.append((timed(v, rng.integers(0, C + 1, n), ts), cut_of(q_hi), G))
    return Case("random 20 steps", _cfg(B, group_cap=C), steps)


def cases() -> List[Case]:
    return [_edges(64), _edges(128),
            _zero_at(128, 2 * 20 + 1, "zero on a lane's last bin"), _zero_at(128, 2 * 21, "zero on a lane's first bin"),
            _threshold(True), _threshold(False), _clipped(), _quiet_after_peak(), _wrap(), _cuts(), _late_record(),
            _shapes(), _hot(False), _hot(True), _random()]


CASE_NAMES = [c.name for c in cases()]


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


def run_pipeline(engine: str, windows: List[np.ndarray], cuts: Sequence[int], n_groups, bins: int, group_cap: int = 8,
                 **kw):
    """The windows through ``WindowPipeline(engine, breach_onset=bins)`` and a ``RingWindowSource`` over a
    span ring, cut at ``cuts`` (0: a cut without a time). Returns (per-window results, per-window
    tracker results (empty with ``bins`` = 0), windows the tracker skipped)."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import Cut, RingWindowSource, WindowPipeline
    from llm_slo_ebpf_toolkit_amd.runtime import load

    rt = load()
    pipe = WindowPipeline(4096, 1024, group_cap, model="bayes", learn=False, user_cap=1024, engine=engine,
                          ttft_slo_ms=SLO, window_ms=160.0, breach_onset=bins, onset_ref_ppm=250_000, **kw)
    ring = rt.HostRing(1 << 12, 64)
    src = RingWindowSource(pipe, None, None, ring)
    res, ons = [], []
    try:
        for w, recs in enumerate(windows):
            G = n_groups if np.isscalar(n_groups) else n_groups[w]
            assert ring.push(recs) == len(recs)
            kk = src.stage(Cut(kernel=0, user=0, spans=ring.head, t_ns=int(cuts[w])), G)["k"]
            res.append({key: np.array(v, copy=True) for key, v in pipe.results(kk, G).items()})
            if bins:
                ons.append({key: np.array(v, copy=True) for key, v in pipe.onset_results(kk, G).items()})
        src.drain()
        skipped = pipe.onset_skipped
    finally:
        pipe.close()
    return res, ons, skipped
