"""Span windows for the TTFT phase split tests (pipeline/retrsli.py, ops/retrsli.py): builders of windows with
the rule's edge values, the named cases both test files run (CASES), and the brute force the oracle is checked
against -- a plain Python loop over the records and a list of the horizon's windows, Python's own round-half-even,
sorted values for the ranks, no histogram rows, no numpy reductions."""

from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.pipeline import retrsli as rs
from tests.decodesli_scenarios import EDGE_US, _lower, brute_bucket

F32 = np.float32
SLO, BUDGET = 800.0, 200.0
SLO_U, BUDGET_U = 80_000, 20_000
UMAX = rs.UNIT_MAX
# the verdict's thresholds of the cases: small counts reach every compare at equality
TH = dict(min_requests=10, coverage_ppm=500_000, budget_ppm=100_000, dominance_ppm=750_000)
# (r, t) in units that land in each cell at SLO_U / BUDGET_U
CELL_RT = ((100, 1_000), (30_000, 40_000), (100, 90_000), (30_000, 120_000), (30_000, 90_000), (15_000, 90_000))


def ms_of(u: int) -> F32:
    """A float32 time in ms whose conversion is exactly ``u`` units (UNIT_MAX: by the clamp)."""
    x = F32(u / 100.0)
    for c in (x, np.nextafter(x, F32(np.inf)), np.nextafter(x, F32(-np.inf))):
        if int(rs.units_of_ms(c)) == u:
            return c
    raise ValueError(f"no float32 ms gives {u} units")


def recs(retr_ms: Sequence[float], ttft_ms: Sequence[float], grp: Sequence[int], flags=0) -> np.ndarray:
    """Span records carrying ``retr_ms`` and ``ttft_ms`` over the flag bits ``flags`` (a value or one per record)."""
    n = len(retr_ms)
    r = np.zeros(n, dtype=R.SPAN)
    r["retr_ms"] = np.asarray(retr_ms, dtype=F32)
    r["ttft_ms"] = np.asarray(ttft_ms, dtype=F32)
    r["group_id"] = np.asarray(grp, dtype=np.uint32)
    r["flags"] = np.asarray(flags, dtype=np.uint32)
    r["ts_ns"] = 1_700_000_000_000_000_000 + np.arange(n)
    r["trace_h"] = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    r["latency_ms"] = np.where(np.isfinite(r["ttft_ms"]), r["ttft_ms"], 0) + 50.0
    return r


def units(r_u: Sequence[int], t_u: Sequence[int], grp: Sequence[int], flags=0) -> np.ndarray:
    """Records whose times convert to exactly ``r_u`` and ``t_u`` units."""
    return recs([ms_of(int(u)) for u in r_u], [ms_of(int(u)) for u in t_u], grp, flags)


def by_cells(g: int, counts: Sequence[int], no_breakdown: int = 0) -> np.ndarray:
    """``counts[c]`` records of service ``g`` in each cell ``c`` and ``no_breakdown`` SLI records without a
    retrieval time (they count in ``sli`` only)."""
    r_u = [CELL_RT[c][0] for c, k in enumerate(counts) for _ in range(k)]
    t_u = [CELL_RT[c][1] for c, k in enumerate(counts) for _ in range(k)]
    parts = [units(r_u, t_u, [g] * len(r_u))]
    if no_breakdown:
        parts.append(recs([0.0] * no_breakdown, [100.0] * no_breakdown, [g] * no_breakdown))
    return np.concatenate(parts)


def mixed_window(rng, n: int, G: int) -> np.ndarray:
    """About ``n`` records of ``G`` services: half of them first-token records with a retrieval time log-normal
    about the service's own median, half final records with SPAN_NO_SLI (a few of those with a late breakdown);
    plus, per service, the compares' two sides and what the rule leaves out or counts aside: start records,
    NaN and negative TTFTs, NaN / zero / negative / too large retrieval times, groups at and above ``G``."""
    g = rng.integers(0, max(G, 1), n)
    first = rng.random(n) < 0.5
    retr = np.where(first | (rng.random(n) < 0.1), rng.lognormal(np.log(60.0 * (1 + g)), 0.6, n), 0.0)
    ttft = retr * (rng.random(n) < 0.95) + rng.lognormal(np.log(350.0), 0.8, n)
    fl = np.where(first, R.SPAN_FIRST_TOKEN, R.SPAN_NO_SLI) | np.where(rng.random(n) < 0.1, R.SPAN_LATE, 0)
    parts = [recs(retr, ttft, g, fl)]
    for s in range(G):
        parts.append(units([BUDGET_U, BUDGET_U + 1, 30_000, 30_000, 1, 0], [90_000, 90_000, 110_000, 110_001, UMAX, UMAX], [s] * 6))
        parts.append(recs([50.0, 50.0, 50.0, 900.0], [F32(SLO), np.nextafter(F32(SLO), F32(np.inf)), F32(-0.0), 100.0], [s] * 4,
                          [0, R.SPAN_NO_SLI, R.SPAN_LATE, R.SPAN_FIRST_TOKEN]))
        parts.append(recs([50.0, np.nan, 0.0, -1.0, 1e7, 50.0], [np.nan, 100.0, 100.0, 900.0, 100.0, -1.0], [s] * 6,
                          [0, 0, R.SPAN_NO_SLI, 0, 0, R.SPAN_NO_SLI]))
    parts.append(recs([50.0, 50.0, 0.0], [100.0, np.nan, 100.0], [G, G + 3, G]))
    parts.append(recs([50.0, 50.0], [100.0, np.nan], [0, 0], [R.SPAN_START | R.SPAN_NO_SLI] * 2))
    out = np.concatenate(parts)
    return out[rng.permutation(len(out))]


# ---- the brute force ----------------------------------------------------------------------------
_BUCKET: Dict[int, int] = {}


def bucket(u: int) -> int:
    b = _BUCKET.get(u)
    if b is None:
        b = _BUCKET[u] = brute_bucket(u)
    return b


def brute_units(ms) -> int:
    """``min(rint(float64(ms) * 100), 2^24 - 1)`` with Python's round (half to even)."""
    x = float(F32(ms)) * 100.0
    return UMAX if x >= UMAX else int(round(x))


def brute_cell(tb: bool, r: int, m: int, slo_u: int, budget_u: int) -> int:
    rb = r > budget_u
    if not tb:
        return 1 if rb else 0
    if m > slo_u:
        return 3 if rb else 2
    return 4 if rb else 5


def brute_state(c: Sequence[int], sli: int, min_requests: int, coverage_ppm: int, budget_ppm: int, dominance_ppm: int) -> int:
    n = sum(c)
    if n < min_requests or n * 10 ** 6 < coverage_ppm * sli:
        return 0
    B, M, R_ = c[2] + c[3] + c[4] + c[5], c[2] + c[3], c[4]
    if B * 10 ** 6 <= budget_ppm * n:
        return 1
    if R_ * 10 ** 6 >= dominance_ppm * B:
        return 2
    if M * 10 ** 6 >= dominance_ppm * B:
        return 3
    return 4


class Brute:
    """The rules record by record: per step a list per service of (r bucket, m bucket, cell, r, t) and its SLI
    count; the horizon is the last ``windows`` of them."""

    def __init__(self, group_cap: int, windows: int, slo_ms: float = SLO, retrieval_budget_ms: float = BUDGET,
                 min_requests: int = 200, coverage_ppm: int = 500_000, budget_ppm: int = 10_000,
                 dominance_ppm: int = 667_000, **_kw):
        self.C, self.W = group_cap, windows
        self.slo = float(F32(slo_ms))
        self.slo_u = brute_units(slo_ms)
        self.budget_u = min(UMAX, max(1, int(round(float(retrieval_budget_ms) * 100.0))))
        self.th = (min_requests, coverage_ppm, budget_ppm, dominance_ppm)
        self.steps: List[Tuple[list, list]] = []
        self.state = [0] * group_cap
        self.age = [0] * group_cap

    @staticmethod
    def _ranks(buckets: List[int]) -> List[int]:
        s = sorted(buckets)
        if not s:
            return [rs.EMPTY] * 4
        return [s[max(1, (q * len(s) + 999) // 1000) - 1] for q in rs.PERMILLE]

    def step(self, records: np.ndarray, n_groups: int) -> Dict[str, np.ndarray]:
        stats = dict.fromkeys(rs.STATS, 0)
        seen: List[list] = [[] for _ in range(self.C)]
        sli = [0] * self.C
        for rec in records:
            fl = int(rec["flags"])
            if fl & R.SPAN_START:
                continue
            g, v, rm = int(rec["group_id"]), float(rec["ttft_ms"]), float(rec["retr_ms"])
            if g >= n_groups:
                stats["out_of_group"] += 1
            elif not v >= 0.0:
                stats["invalid"] += 1
            else:
                if not fl & R.SPAN_NO_SLI:
                    sli[g] += 1
                if not (0.0 < rm < 1e7):
                    stats["no_breakdown"] += 1
                    continue
                stats["observed"] += 1
                stats["extra"] += bool(fl & R.SPAN_NO_SLI)
                r, t = brute_units(rm), brute_units(v)
                stats["exceeds_ttft"] += r > t
                m = t - r if t > r else 0
                seen[g].append((bucket(r), bucket(m), brute_cell(v > self.slo, r, m, self.slo_u, self.budget_u), r, t))
        self.steps.append((seen, sli))
        self.steps = self.steps[-self.W:]
        out = rs.empty_result(self.C)
        for g in range(self.C):
            hor = [x for step, _ in self.steps for x in step[g]]
            for name, rows in (("", seen[g]), ("_roll", hor)):
                for _br, _bm, c, r, t in rows:
                    out["cells" + name][g, c] += 1
                    out["sum_r" + name][g] += np.uint64(r)
                    out["sum_t" + name][g] += np.uint64(t)
                out["q_r_" + ("roll" if name else "win")][g] = self._ranks([x[0] for x in rows])
                out["q_m_" + ("roll" if name else "win")][g] = self._ranks([x[1] for x in rows])
            out["sli"][g] = sli[g]
            out["sli_roll"][g] = sum(s[g] for _, s in self.steps)
            state = brute_state([int(x) for x in out["cells_roll"][g]], int(out["sli_roll"][g]), *self.th)
            self.age[g] = 1 if state != self.state[g] else min(0xFFFFFFFF, self.age[g] + 1)
            self.state[g] = state
            out["state"][g], out["age"][g] = state, self.age[g]
        out["stats"][:len(rs.STATS)] = [stats[name] for name in rs.STATS]
        return out

    def resident(self) -> Dict[str, np.ndarray]:
        rows_r, rows_m = np.zeros((self.C, rs.K), np.uint32), np.zeros((self.C, rs.K), np.uint32)
        cells, sli = np.zeros((self.C, rs.N_CELLS), np.uint32), np.zeros(self.C, np.uint32)
        sums = np.zeros((self.C, 2), np.uint64)
        for step, s in self.steps:
            for g in range(self.C):
                sli[g] += s[g]
                for br, bm, c, r, t in step[g]:
                    rows_r[g, br] += 1
                    rows_m[g, bm] += 1
                    cells[g, c] += 1
                    sums[g] += np.array([r, t], np.uint64)
        return {"rows_r": rows_r, "rows_m": rows_m, "cells": cells, "sli": sli, "sums": sums,
                "state": np.array(self.state, np.uint32), "age": np.array(self.age, np.uint32)}


def same_results(a: dict, b: dict, what: str = "") -> None:
    assert set(a) == set(b) == set(rs.RESULT_FIELDS), what
    for f in rs.RESULT_FIELDS:
        want = np.uint64 if f.startswith("sum_") else np.uint32
        assert a[f].dtype == b[f].dtype == want and a[f].shape == b[f].shape, (what, f, a[f].dtype, b[f].dtype, a[f].shape, b[f].shape)
        np.testing.assert_array_equal(a[f], b[f], err_msg=f"{what} {f}")


RESIDENT = (("rows_r", np.uint32), ("rows_m", np.uint32), ("cells", np.uint32), ("sli", np.uint32), ("sums", np.uint64),
            ("state", np.uint32), ("age", np.uint32))


def same_resident(a: dict, b: dict, what: str = "", pos: bool = True) -> None:
    if pos:
        assert int(a["pos"]) == int(b["pos"]), (what, a["pos"], b["pos"])
    for f, t in RESIDENT:
        assert a[f].dtype == b[f].dtype == t and a[f].shape == b[f].shape, (what, f)
        np.testing.assert_array_equal(a[f], b[f], err_msg=f"{what} resident {f}")


# ---- the named cases ----------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    cfg: dict                                          # group_cap, windows, span_cap, the thresholds
    steps: List[Tuple[np.ndarray, int]]                # (records, n_groups)
    check: Optional[Callable[[List[dict]], None]] = None   # over every step's results (all rows of group_cap)


def _cfg(group_cap=4, windows=2, span_cap=1024, **th):
    return dict(group_cap=group_cap, windows=windows, span_cap=span_cap, slo_ms=SLO, retrieval_budget_ms=BUDGET, **{**TH, **th})


def _stats(res) -> Dict[str, int]:
    return rs.stats_dict(res["stats"])


def _edges_r() -> Case:
    """Every bucket edge as a retrieval time (the TTFT clamps to the largest time, so m = 2^24 - 1 - r), then r = 1,
    r = 2^24 - 1 by the clamp, and a retrieval time just below 1e7 ms (observed) and at it (no breakdown)."""
    us = EDGE_US
    first = units(us, [UMAX] * len(us), [1] * len(us))
    below = np.nextafter(F32(1e7), F32(0))
    second = recs([ms_of(1), ms_of(UMAX), below, F32(1e7)], [100.0] * 4, [0] * 4)

    def check(res):
        assert int(res[0]["cells"][1].sum()) == len(us) and int(res[0]["sum_r"][1]) == sum(us)
        assert int(res[0]["sum_t"][1]) == UMAX * len(us) and _stats(res[0])["observed"] == len(us)
        assert len(us) < 100 and int(res[0]["q_r_win"][1][3]) == rs.K - 1 == brute_bucket(UMAX)
        assert _stats(res[1]) == {"observed": 3, "out_of_group": 0, "invalid": 0, "no_breakdown": 1, "extra": 0, "exceeds_ttft": 2}
        assert int(res[1]["sum_r"][0]) == 1 + 2 * UMAX and res[1]["cells"][0].tolist() == [1, 2, 0, 0, 0, 0]
        assert res[1]["q_r_win"][0].tolist() == [rs.K - 1] * 4 and res[1]["q_m_win"][0].tolist() == [0] + [brute_bucket(9_999)] * 3

    return Case("bucket edges of r, r = 1, the clamp and 1e7", _cfg(), [(first, 2), (second, 2)], check)


def _edges_m() -> Case:
    """Every bucket edge as a model time (r = 100 units), m = 2^24 - 1 (r rounds to 0), and m = 0 from r = t and
    from r > t."""
    us = EDGE_US[:-1]
    first = units([100] * len(us), [u + 100 for u in us], [2] * len(us))
    second = np.concatenate([recs([0.001], [ms_of(UMAX)], [2]), units([500, 501], [500, 500], [2, 2])])

    def check(res):
        assert int(res[0]["sum_t"][2]) - int(res[0]["sum_r"][2]) == sum(us) and _stats(res[0])["exceeds_ttft"] == 0
        assert int(res[0]["q_m_win"][2][3]) == brute_bucket(us[-1]) and int(res[0]["q_r_win"][2][0]) == brute_bucket(100)
        assert _stats(res[1])["observed"] == 3 and _stats(res[1])["exceeds_ttft"] == 1
        assert res[1]["q_m_win"][2].tolist() == [0, rs.K - 1, rs.K - 1, rs.K - 1] and int(res[1]["sum_r"][2]) == 1001

    return Case("bucket edges of m, m = 0 and m = 2^24 - 1", _cfg(), [(first, 3), (second, 3)], check)


def _compares() -> Case:
    """Both sides of each compare: the TTFT at, just below and just above the SLO in float32; m at slo_u and
    slo_u + 1; r at budget_u and budget_u + 1; half-way values that rint sends to even."""
    lo, hi = np.nextafter(F32(SLO), F32(0)), np.nextafter(F32(SLO), F32(np.inf))
    assert int(rs.units_of_ms(lo)) == int(rs.units_of_ms(hi)) == SLO_U  # only the float32 compare tells them apart
    a = recs([10.0] * 3, [F32(SLO), lo, hi], [0] * 3)
    b = units([30_000, 30_000, BUDGET_U, BUDGET_U + 1], [30_000 + SLO_U, 30_001 + SLO_U, 90_000, 90_000], [1] * 4)
    c = recs([0.125, 0.375, 0.625], [100.0] * 3, [2] * 3)

    def check(res):
        assert res[0]["cells"][0].tolist() == [2, 0, 0, 0, 0, 1]
        assert res[0]["cells"][1].tolist() == [0, 0, 0, 1, 2, 1]
        assert int(res[0]["sum_r"][2]) == 12 + 38 + 62

    return Case("both sides of every compare, half to even", _cfg(), [(np.concatenate([a, b, c]), 3)], check)


def _cells() -> Case:
    first = np.concatenate([by_cells(g, [3 * (c == g) for c in range(6)]) for g in range(4)])
    second = np.concatenate([by_cells(0, [0, 0, 0, 0, 2, 0]), by_cells(1, [0, 0, 0, 0, 0, 2]), by_cells(2, [1] * 6)])

    def check(res):
        assert res[0]["cells"].tolist() == [[3 * (c == g) for c in range(6)] for g in range(4)]
        assert res[1]["cells"].tolist() == [[0, 0, 0, 0, 2, 0], [0, 0, 0, 0, 0, 2], [1] * 6, [0] * 6]
        assert res[1]["cells_roll"][2].tolist() == [1, 1, 4, 1, 1, 1]

    return Case("each cell alone in a row, a row with all six", _cfg(), [(first, 4), (second, 4)], check)


def _check_order() -> Case:
    r = recs([50.0, 50.0, 50.0, np.nan, 0.0, -1.0, -0.0, 50.0, 0.0, 50.0],
             [100.0, np.nan, np.nan, 100.0, 100.0, 100.0, 100.0, 100.0, 100.0, 100.0],
             [0, 7, 0, 0, 0, 0, 0, 1, 1, 1],
             [R.SPAN_START | R.SPAN_NO_SLI, 0, 0, 0, 0, 0, 0, R.SPAN_NO_SLI, R.SPAN_NO_SLI, R.SPAN_FIRST_TOKEN])

    def check(res):
        assert _stats(res[0]) == {"observed": 2, "out_of_group": 1, "invalid": 1, "no_breakdown": 5, "extra": 1, "exceeds_ttft": 0}
        assert res[0]["sli"].tolist() == [4, 1, 0, 0] and res[0]["cells"][:, 0].tolist() == [0, 2, 0, 0]

    return Case("check order", _cfg(), [(r, 2)], check)


def _rank_on_lane(last: bool) -> Case:
    """Ten records over bucket 125 (lane 20's last of six) and bucket 126 (lane 21's first), in both histograms (t
    = 2 r, so m = r): rank 5 (p50) falls on the lane's last bucket with five records there, on the next lane's first
    with four."""
    lo, hi = _lower(125), _lower(126)
    k = 5 if last else 4
    us = [lo] * k + [hi] * (10 - k)

    def check(res):
        want = [125 if last else 126, 126, 126, 126]
        assert res[0]["q_r_win"][0].tolist() == want == res[0]["q_m_win"][0].tolist() == res[0]["q_m_roll"][0].tolist()

    return Case(f"rank on a lane's {'last' if last else 'next first'} bucket", _cfg(),
                [(units(us, [2 * u for u in us], [0] * 10), 1)], check)


def _single() -> Case:
    def check(res):
        assert res[0]["q_r_win"][2].tolist() == [brute_bucket(30_000)] * 4 == res[0]["q_r_roll"][2].tolist()
        assert res[0]["q_m_win"][2].tolist() == [brute_bucket(60_000)] * 4 and res[0]["cells"][2].tolist() == [0, 0, 0, 0, 1, 0]
        assert res[0]["q_r_win"][0].tolist() == [rs.EMPTY] * 4 and res[0]["state"].tolist() == [0] * 4

    return Case("n = 1", _cfg(), [(by_cells(2, [0, 0, 0, 0, 1, 0]), 3)], check)


def _states() -> Case:
    """W = 1, so every step's row decides alone: each of the five states reached and left, age growing and
    resetting."""
    rows = [([9, 0, 0, 0, 0, 0], 0), ([9, 0, 0, 0, 1, 0], 1), ([9, 0, 0, 0, 1, 0], 1), ([8, 0, 0, 0, 2, 0], 2),
            ([8, 0, 1, 1, 0, 0], 3), ([8, 0, 1, 0, 1, 0], 4), ([8, 0, 0, 0, 0, 2], 4), ([10, 0, 0, 0, 0, 0], 1), ([0] * 6, 0)]
    steps = [(by_cells(0, c), 1) for c, _ in rows]

    def check(res):
        assert [int(r["state"][0]) for r in res] == [s for _, s in rows]
        assert [int(r["age"][0]) for r in res] == [1, 1, 2, 1, 1, 1, 2, 1, 1]
        assert [int(r["age"][3]) for r in res] == list(range(1, 10)) and all(int(r["state"][3]) == 0 for r in res)

    return Case("every state reached and left", _cfg(windows=1), steps, check)


def _thresholds() -> Case:
    """W = 1; each threshold at equality and one count either side, one service per compare in each step."""
    # min_requests = 10: 9, 10, 11 requests; coverage 1/2: 10 observed of 21, 20, 19 SLI records
    a = [np.concatenate([by_cells(0, [n, 0, 0, 0, 0, 0]), by_cells(1, [10, 0, 0, 0, 0, 0], sli - 10)])
         for n, sli in ((9, 21), (10, 20), (11, 19))]
    # budget 1/10: 1, 2, 3 breaches of 20; dominance 3/4: retrieval 2, 3, 4 of 4 breaches, model 2, 3, 4 of 4
    b = [np.concatenate([by_cells(0, [20 - k, 0, 0, 0, 0, k]), by_cells(1, [20, 0, 0, 0, k + 1, 3 - k]),
                         by_cells(2, [20, 0, k + 1, 0, 0, 3 - k]), by_cells(3, [20, 0, 1, k, 3 - k, 0])]) for k in (1, 2, 3)]

    def check(res):
        assert [r["state"][:2].tolist() for r in res[:3]] == [[0, 0], [1, 1], [1, 1]]
        assert [r["state"].tolist() for r in res[3:]] == [[1, 4, 4, 4], [1, 2, 3, 3], [4, 2, 3, 3]]
        assert res[1]["sli"][:2].tolist() == [10, 20] and res[0]["sli_roll"][:2].tolist() == [9, 21]

    return Case("every threshold at equality and either side", _cfg(windows=1), [(r, 2) for r in a] + [(r, 4) for r in b], check)


def _silence() -> Case:
    """W = 2: service 0 is retrieval bound for three steps (age 1, 2, 3), then silent; its rows roll out and the
    verdict goes back to unknown, where it ages again."""
    busy = by_cells(0, [8, 0, 0, 0, 3, 0])
    steps = [(busy, 1)] * 3 + [(np.zeros(0, R.SPAN), 1)] * 3

    def check(res):
        assert [int(r["state"][0]) for r in res] == [2, 2, 2, 2, 0, 0]
        assert [int(r["age"][0]) for r in res] == [1, 2, 3, 4, 1, 2]
        assert int(res[3]["cells_roll"][0].sum()) == 11 and int(res[4]["cells_roll"][0].sum()) == 0
        assert res[4]["q_r_roll"][0].tolist() == [rs.EMPTY] * 4 and int(res[4]["sum_t_roll"][0]) == 0

    return Case("age grows, a silent service rolls out to unknown", _cfg(), steps, check)


def _horizon(W: int) -> Case:
    """Service 1 goes silent after the second step; step 3 is empty; the group count changes; by the last step
    every window with a record of service 1 has left the horizon."""
    rng = np.random.default_rng(200 + W)
    groups = [3, 3, 2, 3, 0, 1, 3, 3]
    steps = []
    for w, G in enumerate(groups):
        r = np.zeros(0, R.SPAN) if w == 3 else mixed_window(rng, 60, max(G, 1))
        if w >= 2 and len(r):
            r = r[r["group_id"] != 1]
        steps.append((r, G))

    def check(res):
        assert int(res[1]["cells_roll"][1].sum()) > 20 and int(res[2 + W - 1]["cells_roll"][1].sum()) == 0
        assert res[2 + W - 1]["q_m_roll"][1].tolist() == [rs.EMPTY] * 4 and int(res[2 + W - 1]["sli_roll"][1]) == 0
        assert int(res[3]["cells"].sum()) == 0 and int(res[3]["cells_roll"].sum()) > 0
        assert any(int(r["stats"][4]) for r in res) and any(int(r["stats"][5]) for r in res)

    return Case(f"horizon W={W}", _cfg(windows=W), steps, check)


HOT_SPANS = 16_383


def _hot(buckets: int) -> Case:
    """The full span_cap: all records of one service in one (bucket, bucket, cell), or four services with three
    adjacent buckets each."""
    rng = np.random.default_rng(12 + buckets)
    n = HOT_SPANS
    if buckets == 1:
        r = units([30_000], [90_000], [1])[np.zeros(n, np.int64)]
    else:
        g = rng.integers(0, 4, n)
        b0 = brute_bucket(6_000)
        r_u = np.array([_lower(b0 + 8 * int(s) + int(j)) for s, j in zip(g, rng.integers(0, 3, n))])
        m_u = np.array([_lower(brute_bucket(40_000) + int(j)) for j in rng.integers(0, 3, n)])
        r = recs(r_u / 100.0, (r_u + m_u) / 100.0, g, R.SPAN_FIRST_TOKEN)

    def check(res):
        assert int(res[0]["cells"].sum()) == n == _stats(res[0])["observed"] == int(res[0]["sli"].sum())
        if buckets == 1:
            assert res[0]["cells"][1].tolist() == [0, 0, 0, 0, n, 0] and int(res[0]["sum_r"][1]) == 30_000 * n
            assert int(res[0]["sum_t"][1]) == 90_000 * n and int(res[0]["state"][1]) == 2
        else:
            assert int((res[0]["cells"] > 0).sum()) >= 4 and (res[0]["cells"].sum(axis=1) > 3000).all()

    return Case(f"hot {'one key' if buckets == 1 else 'three adjacent buckets'}", _cfg(span_cap=HOT_SPANS), [(r, 4)], check)


def _wide() -> Case:
    """256 services, record i of service i % 256: every workgroup of 256 records holds 6 x 256 = 1,536 keys, more
    than the LDS table's slots, so the fall-through to global memory runs."""
    rng = np.random.default_rng(21)
    n = 3000
    g = np.arange(n) % 256
    r_u = rng.integers(1, 40_000, n)
    r = recs(r_u / 100.0, (r_u + rng.integers(0, 120_000, n)) / 100.0, g)

    def check(res):
        assert int(res[0]["cells"].sum()) == n and int(res[1]["cells_roll"].sum()) == 2 * n
        assert (res[0]["sli"] >= n // 256).all() and int(res[0]["sli"].sum()) == n

    return Case("hot wide: more keys than the table holds", _cfg(group_cap=256, span_cap=4096), [(r, 256), (r[::-1], 256)], check)


def _random() -> Case:
    rng = np.random.default_rng(13)
    steps = []
    for w in range(20):
        G = int(rng.integers(1, 4))
        steps.append((mixed_window(rng, 3000 if w == 7 else int(rng.integers(0, 300)), G), G))
    return Case("hot random 20 steps", _cfg(windows=3, span_cap=4096), steps)


def cases() -> List[Case]:
    return [_edges_r(), _edges_m(), _compares(), _cells(), _check_order(), _rank_on_lane(True), _rank_on_lane(False), _single(),
            _states(), _thresholds(), _silence(), _horizon(2), _horizon(3), _hot(1), _hot(3), _wide(), _random()]


CASE_NAMES = [c.name for c in cases()]


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


def run_pipeline(engine: str, windows: List[np.ndarray], n_groups, horizon: int, group_cap: int = 8, **kw):
    """The windows through ``WindowPipeline(engine, retrieval_sli=horizon)`` and a ``RingWindowSource`` over a
    span ring. Returns (per-window results, per-window tracker results (empty with ``horizon`` = 0))."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import Cut, RingWindowSource, WindowPipeline
    from llm_slo_ebpf_toolkit_amd.runtime import load

    rt = load()
    pipe = WindowPipeline(4096, 1024, group_cap, model="bayes", learn=False, user_cap=1024, engine=engine,
                          ttft_slo_ms=SLO, window_ms=160.0, retrieval_sli=horizon,
                          **{f"retr_{k}": v for k, v in TH.items()}, **kw)
    ring = rt.HostRing(1 << 12, 64)
    src = RingWindowSource(pipe, None, None, ring)
    res, ret = [], []
    try:
        for w, r in enumerate(windows):
            G = n_groups if np.isscalar(n_groups) else n_groups[w]
            assert ring.push(r) == len(r)
            kk = src.stage(Cut(kernel=0, user=0, spans=ring.head, t_ns=1_700_000_000_000_000_000 + w * 160_000_000), G)["k"]
            res.append({key: np.array(v, copy=True) for key, v in pipe.results(kk, G).items()})
            if horizon:
                ret.append({key: np.array(v, copy=True) for key, v in pipe.retrieval_results(kk, G).items()})
        src.drain()
    finally:
        pipe.close()
    return res, ret
