"""Span windows for the decode SLI tests (pipeline/decodesli.py, ops/decodesli.py): builders of windows
with the rule's edge values, the named cases both test files run (CASES), and the brute force the oracle
is checked against -- a plain Python loop over the records and a list of the horizon's windows, sorted
values for the ranks, no histogram rows, no numpy reductions."""

from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.pipeline import decodesli as ds

F32 = np.float32
SLO = 800.0
TPOT_SLO = 100.0
SLO_US = 100_000
GOOD, BAD = 100.0, 900.0
FAST, SLOW = 40_000, 250_000
# equal to the SLO (no breach), just above it and +inf (breaches), -0.0 (observed, no breach), NaN and -1 (invalid)
EDGE_TTFT = [F32(800.0), np.nextafter(F32(800), F32(np.inf)), F32(np.inf), F32(-0.0), F32(np.nan), F32(-1.0)]
EDGE_US = sorted({1, 15, 16, 31, 32, 33, R.SPAN_TPOT_MAX} | {(1 << k) - 1 for k in range(1, 25)} | {1 << k for k in range(24)})


def recs(us: Sequence[int], ttft: Sequence[float], grp: Sequence[int], flags=0) -> np.ndarray:
    """Request spans carrying ``us`` (0: no TPOT) over the flag bits ``flags`` (a value or one per record)."""
    n = len(us)
    r = np.zeros(n, dtype=R.SPAN)
    r["ttft_ms"] = np.asarray(ttft, dtype=F32)
    r["group_id"] = np.asarray(grp, dtype=np.uint32)
    r["flags"] = np.asarray(flags, dtype=np.uint32) | R.pack_tpot_us(np.asarray(us, dtype=np.int64))
    r["ts_ns"] = 1_700_000_000_000_000_000 + np.arange(n)
    r["trace_h"] = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    r["latency_ms"] = np.where(np.isfinite(r["ttft_ms"]), r["ttft_ms"], 0) + 50.0
    return r


def mixed_window(rng, n: int, G: int) -> np.ndarray:
    """About ``n`` finished requests of ``G`` services, each service's TPOT log-normal about its own median,
    plus, per service: every edge TTFT, the SLO's two sides, SPAN_NO_SLI and SPAN_LATE set; and what the rule
    leaves out: start and first-token records (with TPOT bits set), records without a TPOT, groups at and
    above ``G`` with and without one."""
    g = rng.integers(0, max(G, 1), n)
    us = np.clip(rng.lognormal(np.log(30_000.0 * (1 + g)), 0.3, n), 1, R.SPAN_TPOT_MAX).astype(np.int64)
    fl = np.where(rng.random(n) < 0.5, R.SPAN_NO_SLI, 0) | np.where(rng.random(n) < 0.1, R.SPAN_LATE, 0)
    parts = [recs(us, rng.lognormal(np.log(300.0), 1.5, n), g, fl)]
    for s in range(G):
        parts.append(recs([FAST + i for i in range(len(EDGE_TTFT))], EDGE_TTFT, [s] * len(EDGE_TTFT)))
        parts.append(recs([SLO_US, SLO_US + 1, SLO_US - 1, 1, R.SPAN_TPOT_MAX], [GOOD, GOOD, BAD, BAD, GOOD], [s] * 5,
                          [0, R.SPAN_NO_SLI, R.SPAN_LATE, R.SPAN_NO_SLI | R.SPAN_LATE, 0]))
    parts.append(recs([FAST, SLOW, 0, 0], [GOOD, BAD, GOOD, np.nan], [G, G + 3, G, 0]))
    parts.append(recs([FAST, SLOW, 0], [GOOD, np.nan, np.nan], [0, 0, 0],
                      [R.SPAN_FIRST_TOKEN, R.SPAN_START | R.SPAN_NO_SLI, R.SPAN_START | R.SPAN_NO_SLI]))
    out = np.concatenate(parts)
    return out[rng.permutation(len(out))]


# ---- the brute force ----------------------------------------------------------------------------
def brute_bucket(u: int) -> int:
    """The bucket by search over ``lower``: the last bucket whose lower edge is at or below ``u``."""
    b = 0
    while b + 1 < ds.K and _lower(b + 1) <= u:
        b += 1
    return b


def _lower(b: int) -> int:
    return b if b < 16 else (16 + b % 16) << (b // 16 - 1)


class Brute:
    """The rules record by record: per step a list per service of (bucket, cell, u); the horizon is the
    last ``windows`` of them."""

    def __init__(self, group_cap: int, windows: int, slo_ms: float = SLO, tpot_slo_ms: float = TPOT_SLO, **_kw):
        self.C, self.W = group_cap, windows
        self.slo = float(F32(slo_ms))
        self.slo_us = min(R.SPAN_TPOT_MAX, max(1, int(tpot_slo_ms * 1000 + 0.5)))
        self.steps: List[List[List[Tuple[int, int, int]]]] = []

    @staticmethod
    def _ranks(buckets: List[int]) -> List[int]:
        s = sorted(buckets)
        if not s:
            return [ds.EMPTY] * 4
        return [s[max(1, (q * len(s) + 999) // 1000) - 1] for q in ds.PERMILLE]

    def step(self, records: np.ndarray, n_groups: int) -> Dict[str, np.ndarray]:
        stats = dict.fromkeys(ds.STATS, 0)
        seen: List[List[Tuple[int, int, int]]] = [[] for _ in range(self.C)]
        for r in records:
            fl = int(r["flags"])
            if fl & (R.SPAN_START | R.SPAN_FIRST_TOKEN):
                continue
            u, g, v = fl >> 8, int(r["group_id"]), float(r["ttft_ms"])
            if u == 0:
                stats["no_decode"] += 1
            elif g >= n_groups:
                stats["out_of_group"] += 1
            elif not v >= 0.0:
                stats["invalid"] += 1
            else:
                stats["observed"] += 1
                seen[g].append((brute_bucket(u), int(v > self.slo) + 2 * int(u > self.slo_us), u))
        self.steps.append(seen)
        self.steps = self.steps[-self.W:]
        out = ds.empty_result(self.C)
        for g in range(self.C):
            hor = [x for step in self.steps for x in step[g]]
            for name, rows in (("", seen[g]), ("_roll", hor)):
                for _b, c, u in rows:
                    out["cells" + name][g, c] += 1
                    out["sum_us" + name][g] += np.uint64(u)
            out["q_win"][g] = self._ranks([b for b, _c, _u in seen[g]])
            out["q_roll"][g] = self._ranks([b for b, _c, _u in hor])
        out["stats"][:len(ds.STATS)] = [stats[name] for name in ds.STATS]
        return out

    def resident(self) -> Dict[str, np.ndarray]:
        rows, cells = np.zeros((self.C, ds.K), np.uint32), np.zeros((self.C, ds.N_CELLS), np.uint32)
        sums = np.zeros(self.C, np.uint64)
        for step in self.steps:
            for g in range(self.C):
                for b, c, u in step[g]:
                    rows[g, b] += 1
                    cells[g, c] += 1
                    sums[g] += np.uint64(u)
        return {"rows": rows, "cells": cells, "sum_us": sums}


_DTYPES = {"sum_us": np.uint64, "sum_us_roll": np.uint64}


def same_results(a: dict, b: dict, what: str = "") -> None:
    assert set(a) == set(b) == set(ds.RESULT_FIELDS), what
    for f in ds.RESULT_FIELDS:
        want = _DTYPES.get(f, np.uint32)
        assert a[f].dtype == b[f].dtype == want and a[f].shape == b[f].shape, (what, f, a[f].dtype, b[f].dtype, a[f].shape, b[f].shape)
        np.testing.assert_array_equal(a[f], b[f], err_msg=f"{what} {f}")


def same_resident(a: dict, b: dict, what: str = "", pos: bool = True) -> None:
    if pos:
        assert int(a["pos"]) == int(b["pos"]), (what, a["pos"], b["pos"])
    for f, t in (("rows", np.uint32), ("cells", np.uint32), ("sum_us", np.uint64)):
        assert a[f].dtype == b[f].dtype == t and a[f].shape == b[f].shape, (what, f)
        np.testing.assert_array_equal(a[f], b[f], err_msg=f"{what} resident {f}")


# ---- the named cases ----------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    cfg: dict                                          # group_cap, windows, span_cap
    steps: List[Tuple[np.ndarray, int]]                # (records, n_groups)
    check: Optional[Callable[[List[dict]], None]] = None   # over every step's results (all rows of group_cap)


def _cfg(group_cap=3, windows=2, span_cap=1024):
    return dict(group_cap=group_cap, windows=windows, span_cap=span_cap, slo_ms=SLO, tpot_slo_ms=TPOT_SLO)


def _bucket_edges() -> Case:
    us = EDGE_US
    first = recs(us, [GOOD] * len(us), [1] * len(us))
    second = recs(us[::2], [GOOD] * len(us[::2]), [0] * len(us[::2]))

    def check(res):
        assert int(res[0]["cells"][1].sum()) == len(us) and int(res[0]["sum_us"][1]) == sum(us)
        assert int(res[0]["stats"][0]) == len(us) and int(res[1]["cells_roll"].sum()) == len(us) + len(us[::2])
        # fewer than 100 records: p99 is the largest, in the last bucket
        assert len(us) < 100 and int(res[0]["q_win"][1][3]) == ds.K - 1 == brute_bucket(R.SPAN_TPOT_MAX)

    return Case("bucket edges", _cfg(), [(first, 2), (second, 2)], check)


def _rank_on_lane(last: bool) -> Case:
    """Ten records over bucket 125 (lane 20's last of six) and bucket 126 (lane 21's first): rank 5 (p50)
    falls on the lane's last bucket with five records there, on the next lane's first with four."""
    lo, hi = _lower(125), _lower(126)
    k = 5 if last else 4
    us = [lo] * k + [hi] * (10 - k)

    def check(res):
        assert res[0]["q_win"][0].tolist() == [125 if last else 126, 126, 126, 126]

    return Case(f"rank on a lane's {'last' if last else 'next first'} bucket", _cfg(), [(recs(us, [GOOD] * 10, [0] * 10), 1)], check)


def _single() -> Case:
    def check(res):
        assert res[0]["q_win"][2].tolist() == [brute_bucket(SLOW)] * 4 == res[0]["q_roll"][2].tolist()
        assert res[0]["cells"][2].tolist() == [0, 0, 1, 0] and res[0]["q_win"][0].tolist() == [ds.EMPTY] * 4

    return Case("n = 1", _cfg(), [(recs([SLOW], [GOOD], [2]), 3)], check)


def _slo_sides() -> Case:
    above = np.nextafter(F32(SLO), F32(np.inf))
    r = recs([SLO_US, SLO_US + 1, SLO_US, SLO_US + 1], [F32(SLO), F32(SLO), above, above], [0] * 4)

    def check(res):
        assert res[0]["cells"][0].tolist() == [1, 1, 1, 1]

    return Case("both sides of both SLOs", _cfg(), [(r, 1)], check)


def _check_order() -> Case:
    r = recs([0, FAST, FAST, 0, FAST, FAST], [GOOD, GOOD, np.nan, np.nan, np.nan, -1.0], [7, 7, 0, 0, 7, 1])

    def check(res):
        assert ds.stats_dict(res[0]["stats"]) == {"observed": 0, "invalid": 2, "out_of_group": 2, "no_decode": 2}

    return Case("check order", _cfg(), [(r, 2)], check)


def _flags() -> Case:
    fl = [R.SPAN_START | R.SPAN_NO_SLI, R.SPAN_FIRST_TOKEN, R.SPAN_FIRST_TOKEN | R.SPAN_LATE, R.SPAN_NO_SLI, 0, R.SPAN_LATE,
          R.SPAN_NO_SLI | R.SPAN_LATE, 0xF0]
    r = recs([FAST] * len(fl), [GOOD] * len(fl), [0] * len(fl), fl)

    def check(res):
        assert ds.stats_dict(res[0]["stats"]) == {"observed": 5, "invalid": 0, "out_of_group": 0, "no_decode": 0}
        assert res[0]["cells"][0].tolist() == [5, 0, 0, 0]

    return Case("start and first-token skipped, NO_SLI either way", _cfg(), [(r, 1)], check)


def _horizon(W: int) -> Case:
    """Service 1 goes silent after the second step; step 3 is empty; the group count changes; by the last
    step every window with a record of service 1 has left the horizon."""
    rng = np.random.default_rng(100 + W)
    groups = [3, 3, 2, 3, 0, 1, 3, 3]
    steps = []
    for w, G in enumerate(groups):
        r = np.zeros(0, R.SPAN) if w == 3 else mixed_window(rng, 60, max(G, 1))
        if w >= 2 and len(r):
            r = r[r["group_id"] != 1]
        steps.append((r, G))

    def check(res):
        assert int(res[1]["cells_roll"][1].sum()) > 20 and int(res[2 + W - 1]["cells_roll"][1].sum()) == 0
        assert res[2 + W - 1]["q_roll"][1].tolist() == [ds.EMPTY] * 4 and int(res[2 + W - 1]["sum_us_roll"][1]) == 0
        assert int(res[3]["cells"].sum()) == 0 and int(res[3]["cells_roll"].sum()) > 0

    return Case(f"horizon W={W}", _cfg(windows=W), steps, check)


def _hot(buckets: int) -> Case:
    """4096 records of one service in one bucket, or over three adjacent ones."""
    rng = np.random.default_rng(12 + buckets)
    b0 = brute_bucket(60_000)
    us = np.array([_lower(b0 + int(j)) for j in rng.integers(0, buckets, 4096)]) + rng.integers(0, 100, 4096)
    v = rng.lognormal(np.log(600.0), 1.0, 4096).astype(F32)
    r = recs(us, v, np.ones(4096, np.int64))

    def check(res):
        assert int(res[0]["cells"][1].sum()) == 4096 and int(res[0]["cells"][1][1]) == int((v > F32(SLO)).sum()) > 500
        assert int(res[0]["sum_us"][1]) == int(us.sum()) and b0 <= int(res[0]["q_win"][1][0]) < b0 + buckets

    return Case(f"hot {'one bucket' if buckets == 1 else 'three buckets'}", _cfg(group_cap=2, span_cap=4096), [(r, 2)], check)


def _wide() -> Case:
    """8 services x 64 buckets: 512 histogram keys, 32 cells and 8 sums into a table of 256 slots."""
    rng = np.random.default_rng(21)
    n = 3000
    b0 = brute_bucket(20_000)  # 64 buckets from here straddle the TPOT SLO
    us = np.array([_lower(b0 + int(j)) for j in rng.integers(0, 64, n)])
    r = recs(us, np.where(rng.random(n) < 0.3, BAD, GOOD), rng.integers(0, 8, n))

    def check(res):
        assert int(res[0]["cells"].sum()) == n and int(res[1]["cells_roll"].sum()) == 2 * n
        assert int((res[0]["cells"] > 0).sum()) == 32

    return Case("hot wide: more keys than the table holds", _cfg(group_cap=8, span_cap=4096), [(r, 8), (r[::-1], 8)], check)


def _random() -> Case:
    rng = np.random.default_rng(13)
    steps = []
    for w in range(5):
        G = int(rng.integers(1, 6))
        steps.append((mixed_window(rng, 3000 if w == 1 else int(rng.integers(0, 300)), G), G))
    return Case("hot random 3000", _cfg(group_cap=5, windows=3, span_cap=4096), steps)


def cases() -> List[Case]:
    return [_bucket_edges(), _rank_on_lane(True), _rank_on_lane(False), _single(), _slo_sides(), _check_order(), _flags(),
            _horizon(2), _horizon(3), _hot(1), _hot(3), _wide(), _random()]


CASE_NAMES = [c.name for c in cases()]


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


def run_pipeline(engine: str, windows: List[np.ndarray], n_groups, horizon: int, group_cap: int = 8, **kw):
    """The windows through ``WindowPipeline(engine, decode_sli=horizon)`` and a ``RingWindowSource`` over a
    span ring. Returns (per-window results, per-window tracker results (empty with ``horizon`` = 0))."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import Cut, RingWindowSource, WindowPipeline
    from llm_slo_ebpf_toolkit_amd.runtime import load

    rt = load()
    pipe = WindowPipeline(4096, 1024, group_cap, model="bayes", learn=False, user_cap=1024, engine=engine,
                          ttft_slo_ms=SLO, window_ms=160.0, decode_sli=horizon, tpot_slo_ms=TPOT_SLO, **kw)
    ring = rt.HostRing(1 << 12, 64)
    src = RingWindowSource(pipe, None, None, ring)
    res, dec = [], []
    try:
        for w, r in enumerate(windows):
            G = n_groups if np.isscalar(n_groups) else n_groups[w]
            assert ring.push(r) == len(r)
            kk = src.stage(Cut(kernel=0, user=0, spans=ring.head, t_ns=1_700_000_000_000_000_000 + w * 160_000_000), G)["k"]
            res.append({key: np.array(v, copy=True) for key, v in pipe.results(kk, G).items()})
            if horizon:
                dec.append({key: np.array(v, copy=True) for key, v in pipe.decode_results(kk, G).items()})
        src.drain()
    finally:
        pipe.close()
    return res, dec
