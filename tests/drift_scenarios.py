"""Span windows for the TTFT drift tests (pipeline/drift.py, ops/drift.py): builders of windows with
records in chosen buckets, the named cases both test files run (CASES), and the brute force the oracle
is checked against -- it keeps no histogram: per service the raw values' bucket ids (found by a search
over the bucket edges, not by the bit rule) as sorted lists, windows as a plain list (no ring position,
no stale row), Python integers for every product.

The shapes are tiny on purpose (R = 2, L = 1, B = 3, group_cap 3-5): the kernel's errors live at lane and
ring boundaries, not at scale. With R = 2, L = 1 the window of step i leaves the gap at step i + 3."""

import bisect
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.pipeline import drift as dr
from llm_slo_ebpf_toolkit_amd.pipeline import slisketch as sk

F32 = np.float32
EDGES = [float(e) for e in sk.bucket_edges()]   # EDGES[b - 1] is bucket b's lower edge, b in 1..384; EDGES[384] = 2^21
EMPTY = dr.EMPTY


def val(b: int, top: bool = False) -> np.float32:
    """A float32 in bucket ``b``: its lower edge, or with ``top`` the largest value below the next edge."""
    if b == 0:
        return F32(0.0) if not top else np.nextafter(F32(EDGES[0]), F32(0))
    if b == dr.K - 1:
        return F32(EDGES[-1]) if not top else F32(np.inf)
    return F32(EDGES[b - 1]) if not top else np.nextafter(F32(EDGES[b]), F32(0))


def recs(values: Sequence[float], grp: Sequence[int], flags=0) -> np.ndarray:
    n = len(values)
    r = np.zeros(n, dtype=R.SPAN)
    r["ttft_ms"] = np.asarray(values, dtype=F32)
    r["group_id"] = np.asarray(grp, dtype=np.uint32)
    r["flags"] = np.asarray(flags, dtype=np.uint32)
    r["ts_ns"] = 1_700_000_000_000_000_000 + np.arange(n)
    r["trace_h"] = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    r["latency_ms"] = np.where(np.isfinite(r["ttft_ms"]), r["ttft_ms"], 0) + 50.0
    return r


def win(spec: Dict[int, Dict[int, int]]) -> np.ndarray:
    """A window with, per service, ``count`` records in each bucket: {service: {bucket: count}}; the
    records of a bucket alternate between its lowest and its highest value."""
    v, g = [], []
    for s, hist in spec.items():
        for b, n in hist.items():
            v += [val(b, top=bool(j & 1)) for j in range(n)]
            g += [s] * n
    return recs(v, g) if v else np.zeros(0, R.SPAN)


def lognormal_window(rng, rate: float, median: float, G: int = 1, sigma: float = 0.25) -> np.ndarray:
    """The generator the defaults were reasoned with: per service a Poisson(rate) number of TTFTs,
    log-normal about ``median``, cast to float32."""
    parts = []
    for s in range(G):
        n = int(rng.poisson(rate))
        parts.append(recs(rng.lognormal(np.log(median), sigma, n).astype(F32), [s] * n))
    return np.concatenate(parts) if parts else np.zeros(0, R.SPAN)


def mixed_window(rng, n: int, G: int, medians: Sequence[float]) -> np.ndarray:
    """About ``n`` records of ``G`` services, each log-normal about its median, plus what the rule leaves
    out or counts apart: NaN and negatives (invalid), -0.0, +inf, SPAN_NO_SLI records, SPAN_LATE ones
    (counted), groups at and above ``G``."""
    g = rng.integers(0, max(G, 1), n)
    v = rng.lognormal(np.log(np.asarray(medians, dtype=np.float64)[g % len(medians)]), 0.3, n)
    fl = np.where(rng.random(n) < 0.2, R.SPAN_NO_SLI, 0) | np.where(rng.random(n) < 0.1, R.SPAN_LATE, 0)
    parts = [recs(v, g, fl)]
    for s in range(G):
        parts.append(recs([np.nan, -1.0, -0.0, np.inf, 0.1, 3e6], [s] * 6))
    parts.append(recs([100.0, np.nan, 200.0], [G, G + 3, G], [0, 0, R.SPAN_NO_SLI]))
    out = np.concatenate(parts)
    return out[rng.permutation(len(out))]


# ---- the brute force ----------------------------------------------------------------------------
def brute_bucket(v: float) -> int:
    """The bucket by search over the edges: 0 below 0.125 ms, else the number of edges at or below ``v``."""
    return bisect.bisect_right(EDGES, float(v))


def brute_statistic(recent: List[int], base: List[int]) -> Tuple[int, int, int, int]:
    """(slow_num, fast_num, slow_at, fast_at) of two sorted lists of bucket ids. The difference only
    changes at a bucket that holds a record, so the first bucket attaining a positive maximum is one."""
    n_r, n_b = len(recent), len(base)
    best = [0, 0]
    at = [EMPTY, EMPTY]
    for k in sorted(set(recent) | set(base)):
        d = bisect.bisect_right(base, k) * n_r - bisect.bisect_right(recent, k) * n_b
        for j, e in enumerate((d, -d)):
            if e > best[j]:
                best[j], at[j] = e, k
    return best[0], best[1], at[0], at[1]


def brute_ranks(buckets: List[int]) -> List[int]:
    if not buckets:
        return [EMPTY] * 4
    return [buckets[max(1, (q * len(buckets) + 999) // 1000) - 1] for q in dr.PERMILLE]


class Brute:
    """The rules window by window: ``wins`` is every step's per-service sorted bucket list; the recent
    sample is the last R of them, the baseline a list of admitted windows (at most B, oldest first)."""

    def __init__(self, group_cap: int, recent: int, gap: int, baseline: int, crit=None, min_shift=None, min_recent=None,
                 min_base=None, min_base_windows=None, hold_max=None, **_kw):
        self.C, self.R, self.L, self.B = group_cap, recent, gap, baseline
        self.crit_q = int(np.floor((4.0 if crit is None else crit) * 2.0 ** 32 + 0.5))
        self.s = 2 if min_shift is None else min_shift
        self.min_recent = 30 if min_recent is None else min_recent
        self.min_base = 100 if min_base is None else min_base
        self.min_windows = min(baseline, 10) if min_base_windows is None else min_base_windows
        self.hold_max = 4 * baseline if hold_max is None else hold_max
        self.wins: List[List[List[int]]] = []
        self.base: List[List[List[int]]] = [[] for _ in range(group_cap)]
        self.admissions = [0] * group_cap
        self.hold = [0] * group_cap
        self.prev = [0] * group_cap

    def step(self, records: np.ndarray, n_groups: int) -> Dict[str, np.ndarray]:
        stats = dict.fromkeys(dr.STATS, 0)
        cur: List[List[int]] = [[] for _ in range(self.C)]
        for r in records:
            if int(r["flags"]) & R.SPAN_NO_SLI:
                continue
            g, v = int(r["group_id"]), float(r["ttft_ms"])
            if g >= n_groups:
                stats["out_of_group"] += 1
            elif not v >= 0.0:
                stats["invalid"] += 1
            else:
                stats["observed"] += 1
                cur[g].append(brute_bucket(v))
        self.wins.append([sorted(c) for c in cur])
        i = len(self.wins) - 1
        out = dr.empty_result(self.C)
        for g in range(self.C):
            if i >= self.R + self.L:
                x = self.wins[i - self.R - self.L][g]
                if x and not self.prev[g] & dr.SLOW:
                    self.base[g] = (self.base[g] + [x])[-self.B:]
                    self.admissions[g] += 1
                    stats["admitted"] += 1
                elif x:
                    stats["withheld"] += 1
            rec = sorted(b for w in self.wins[max(0, i - self.R + 1):] for b in w[g])
            bas = sorted(b for w in self.base[g] for b in w)
            n_r, n_b, fill = len(rec), len(bas), len(self.base[g])
            sn, fn, sa, fa = brute_statistic(rec, bas)
            qr, qb = brute_ranks(rec), brute_ranks(bas)
            if n_r < max(self.min_recent, 1) or n_b < max(self.min_base, 1) or fill < self.min_windows:
                st = dr.WARMING
            else:
                nn, ne = n_r * n_b, (n_r * n_b) // (n_r + n_b)
                st = 0
                if ((sn << 16) // nn) ** 2 * ne > self.crit_q and (qr[0] >= qb[0] + self.s or qr[1] >= qb[1] + self.s):
                    st |= dr.SLOW
                if ((fn << 16) // nn) ** 2 * ne > self.crit_q and (qb[0] >= qr[0] + self.s or qb[1] >= qr[1] + self.s):
                    st |= dr.FAST
            self.hold[g] = self.hold[g] + 1 if st & dr.SLOW else 0
            if self.hold[g] >= self.hold_max:
                st, self.hold[g], self.base[g] = dr.WARMING | dr.REBASED, 0, []
                stats["rebased"] += 1
            self.prev[g] = st
            for name, x in (("n_win", len(cur[g])), ("n_recent", n_r), ("n_base", n_b), ("base_fill", fill), ("slow_num", sn),
                            ("fast_num", fn), ("slow_at", sa), ("fast_at", fa), ("state", st), ("hold", self.hold[g])):
                out[name][g] = x
            out["q_recent"][g], out["q_base"][g] = qr, qb
        out["stats"][:len(dr.STATS)] = [stats[name] for name in dr.STATS]
        return out

    def resident(self) -> Dict[str, np.ndarray]:
        rows = {k: np.zeros((self.C, dr.ROW_STRIDE), np.uint32) for k in ("recent", "base")}
        i = len(self.wins) - 1
        for g in range(self.C):
            for w in self.wins[max(0, i - self.R + 1):]:
                for b in w[g]:
                    rows["recent"][g, b] += 1
            for w in self.base[g]:
                for b in w:
                    rows["base"][g, b] += 1
        u = lambda a: np.asarray(a, dtype=np.uint32)  # noqa: E731
        return {**rows, "base_fill": u([len(b) for b in self.base]), "base_pos": u(self.admissions), "hold": u(self.hold),
                "pos": len(self.wins) % (self.R + self.L)}


_DTYPES = {"slow_num": np.uint64, "fast_num": np.uint64}


def same_results(a: dict, b: dict, what: str = "") -> None:
    assert set(a) == set(b) == set(dr.RESULT_FIELDS), what
    for f in dr.RESULT_FIELDS:
        want = _DTYPES.get(f, np.uint32)
        assert a[f].dtype == b[f].dtype == want and a[f].shape == b[f].shape, (what, f, a[f].dtype, b[f].dtype, a[f].shape, b[f].shape)
        np.testing.assert_array_equal(a[f], b[f], err_msg=f"{what} {f}")


def same_resident(a: dict, b: dict, what: str = "") -> None:
    assert int(a["pos"]) == int(b["pos"]), (what, a["pos"], b["pos"])
    for f in ("recent", "base", "base_fill", "base_pos", "hold"):
        assert a[f].dtype == b[f].dtype == np.uint32 and a[f].shape == b[f].shape, (what, f)
        np.testing.assert_array_equal(a[f], b[f], err_msg=f"{what} resident {f}")


# ---- the named cases ----------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    cfg: dict
    steps: List[Tuple[np.ndarray, int]]                # (records, n_groups)
    check: Optional[Callable[[List[dict]], None]] = None   # over every step's results (all rows of group_cap)


def _cfg(group_cap=3, span_cap=256, **kw):
    c = dict(group_cap=group_cap, span_cap=span_cap, recent=2, gap=1, baseline=3, crit=4.0, min_shift=2, min_recent=2,
             min_base=2, min_base_windows=1, hold_max=3)
    c.update(kw)
    return c


def _pair_steps(base: Dict[int, int], recent: Dict[int, int], g: int = 1, G: int = 3) -> List[Tuple[np.ndarray, int]]:
    """Four steps after which service g's baseline is ``base`` (step 0's window, admitted at step 3) and its
    recent sample is ``recent`` (step 3's window; steps 1 and 2 are empty)."""
    e = np.zeros(0, R.SPAN)
    return [(win({g: base}), G), (e, G), (e, G), (win({g: recent}), G)]


def _row(res, g: int = 1) -> dict:
    return {k: (res[k][g].tolist() if res[k].ndim > 1 else int(res[k][g])) for k in dr.RESULT_FIELDS if k != "stats"}


def _identical() -> Case:
    h = {100: 7, 101: 5, 230: 8}

    def check(res):
        r = _row(res[3])
        assert (r["slow_num"], r["fast_num"], r["slow_at"], r["fast_at"]) == (0, 0, EMPTY, EMPTY)
        assert r["state"] == 0 and r["n_recent"] == r["n_base"] == 20 and r["q_recent"] == r["q_base"]
        assert _row(res[2])["state"] == dr.WARMING and _row(res[3], 0)["state"] == dr.WARMING

    return Case("identical rows", _cfg(), _pair_steps(h, h), check)


def _disjoint() -> Case:
    def check(res):
        r = _row(res[3])
        assert (r["slow_num"], r["slow_at"], r["fast_num"], r["fast_at"]) == (100, 100, 0, EMPTY) and r["state"] == dr.SLOW
        assert r["hold"] == 1

    return Case("disjoint rows", _cfg(), _pair_steps({100: 10}, {200: 10}), check)


def _max_at(k: int, fast: bool = False) -> Case:
    """The maximum on bucket ``k``: one sample has 5 records in k - 1 and 5 in k (10 in bucket 0 for k = 0),
    the other 10 in k + 1, so the difference is 50 at k - 1, 100 at k and 0 from k + 1 on. The medians lie two
    buckets apart (one for k = 0, which therefore stays calm with s = 2)."""
    lo = {k - 1: 5, k: 5} if k else {0: 10}
    hi = {k + 1: 10}
    base, recent = (hi, lo) if fast else (lo, hi)

    def check(res):
        r = _row(res[3])
        num, at, other, oat = ("fast_num", "fast_at", "slow_num", "slow_at") if fast else ("slow_num", "slow_at", "fast_num", "fast_at")
        assert (r[num], r[at], r[other], r[oat]) == (100, k, 0, EMPTY), r
        assert r["state"] == (0 if k == 0 else dr.FAST if fast else dr.SLOW)

    lane = f"lane {k // 7}'s {'last' if k % 7 == 6 else 'first' if k % 7 == 0 else 'inner'} bucket"
    return Case(f"{'fast' if fast else 'slow'} maximum at bucket {k} ({lane})", _cfg(), _pair_steps(base, recent), check)


def _last_bucket() -> Case:
    """At the last bucket both cumulative counts are the totals, so the difference is 0 there whatever the
    rows hold: with records in bucket 385 the maximum sits on the bucket before it. Service 1 slow, 2 fast."""
    e = np.zeros(0, R.SPAN)
    steps = [(win({1: {384: 10}, 2: {385: 10}}), 3), (e, 3), (e, 3), (win({1: {385: 10}, 2: {384: 10}}), 3)]

    def check(res):
        a, b = _row(res[3], 1), _row(res[3], 2)
        assert (a["slow_num"], a["slow_at"], a["fast_at"]) == (100, 384, EMPTY) and a["q_recent"] == [385] * 4
        assert (b["fast_num"], b["fast_at"], b["slow_at"]) == (100, 384, EMPTY) and b["q_base"] == [385] * 4

    return Case("records in bucket 385: the maximum at 384", _cfg(), steps, check)


def _tie(same_lane: bool) -> Case:
    """The difference is 50 at the first bucket, 0 at the second, 50 at the third, 0 at the fourth: a tie
    that must resolve to the first, across two lanes (10 | 20) or within one (14 .. 17)."""
    b = [14, 15, 16, 17] if same_lane else [10, 15, 20, 25]

    def check(res):
        r = _row(res[3])
        assert (r["slow_num"], r["slow_at"], r["fast_num"]) == (50, b[0], 0), r

    return Case(f"tie resolves to the first bucket ({'one lane' if same_lane else 'two lanes'})", _cfg(),
                _pair_steps({b[0]: 5, b[2]: 5}, {b[1]: 5, b[3]: 5}), check)


def _crit_edge(above: bool) -> Case:
    """Disjoint rows of 10: Dq = 2^16, n_e = 5, so Dq Dq n_e = 5 * 2^32. With c^2 = 5 that equals crit_q (not
    significant); with c^2 = 5 - 2^-32 it is one above it (significant). Both are exact in float64."""
    c2 = 5.0 - 2.0 ** -32 if above else 5.0
    assert dr.crit_q(c2) == 5 * 2 ** 32 - (1 if above else 0)

    def check(res):
        r = _row(res[3])
        assert r["slow_num"] == 100 and r["state"] == (dr.SLOW if above else 0), r

    return Case(f"Dq Dq n_e {'one above' if above else 'equal to'} crit_q", _cfg(crit=c2), _pair_steps({100: 10}, {200: 10}), check)


def _shift(d: int, on_p90: bool) -> Case:
    """40 records a side, half in bucket 100, half in 300 (p50 = 100, p90 = 300): D = 1/2, n_e = 20,
    D^2 n_e = 5 > 4, significant. The recent sample's lower half (p50) or upper half (p90) lies ``d``
    buckets higher; s = 2."""
    recent = {100: 20, 300 + d: 20} if on_p90 else {100 + d: 20, 300: 20}

    def check(res):
        r = _row(res[3])
        assert r["q_base"][:2] == [100, 300] and r["q_recent"][:2] == ([100, 300 + d] if on_p90 else [100 + d, 300])
        assert r["slow_num"] == 800 and r["state"] == (dr.SLOW if d >= 2 else 0), r

    return Case(f"shift of {d} buckets on {'p90' if on_p90 else 'p50'} only", _cfg(), _pair_steps({100: 20, 300: 20}, recent), check)


def _threshold(which: str, below: bool) -> Case:
    """Each ``min_*`` threshold at its value (decided) and one below it (warming)."""
    n = 19 if below else 20
    if which == "min_recent":
        cfg, steps, at = _cfg(min_recent=20), _pair_steps({100: 20}, {200: n}), 3
    elif which == "min_base":
        cfg, steps, at = _cfg(min_base=20), _pair_steps({100: n}, {200: 20}), 3
    else:  # two baseline windows by step 4, one at step 3
        e = np.zeros(0, R.SPAN)
        cfg, at = _cfg(min_base_windows=2), 3 if below else 4
        steps = [(win({1: {100: 10}}), 3), (win({1: {100: 10}}), 3), (e, 3), (win({1: {200: 20}}), 3), (e, 3)]

    def check(res):
        r = _row(res[at])
        assert r["slow_num"] > 0 and r["state"] == (dr.WARMING if below else dr.SLOW), r

    return Case(f"{which} {'one below' if below else 'at'} its value", cfg, steps, check)


def _rings() -> Case:
    """Ten distinct windows (3 + i records in bucket 50 + i), never significant (a huge c^2): every window
    leaves the recent sample after R steps, the gap after R + L and the full baseline ring after B more."""
    n = lambda i: 3 + i  # noqa: E731
    steps = [(win({1: {50 + i: n(i)}, 0: {60: 2}}), 3) for i in range(10)]

    def check(res):
        for i, r in enumerate(res):
            assert int(r["n_win"][1]) == n(i) and int(r["n_recent"][1]) == n(i) + (n(i - 1) if i else 0)
            left = list(range(0, i - 2))[-3:]   # the windows that left the gap, the last B of them
            assert int(r["n_base"][1]) == sum(n(j) for j in left) and int(r["base_fill"][1]) == len(left)
            assert int(r["state"][1]) == (dr.WARMING if i < 3 else 0)
            assert int(r["stats"][3]) == (2 if i >= 3 else 0)
        assert res[9]["q_base"][1].tolist()[0] == 50 + 5   # windows 4, 5, 6: 7 + 8 + 9 records, rank 12 in the second

    return Case("windows leave recent, the gap and a full baseline ring", _cfg(crit=1e6), steps, check)


def _empty_not_admitted() -> Case:
    a, e = win({1: {100: 10}}), np.zeros(0, R.SPAN)
    steps = [(a, 3), (e, 3), (a, 3), (a, 3), (a, 3), (a, 3)]

    def check(res):
        assert [int(r["base_fill"][1]) for r in res] == [0, 0, 0, 1, 1, 2]
        assert [int(r["stats"][3]) for r in res] == [0, 0, 0, 1, 0, 1] and all(int(r["stats"][4]) == 0 for r in res)

    return Case("an empty window is not admitted", _cfg(), steps, check)


def _withheld() -> Case:
    """Calm A windows, two slow S windows, calm again (hold_max out of reach). Step 4 turns slow (p90 of A + S
    is S's bucket), so the windows leaving the gap at steps 5, 6 and 7 are withheld; step 7 is calm again, and
    the window leaving at step 8 is admitted."""
    a, s = win({1: {100: 20}}), win({1: {200: 20}})
    steps = [(x, 3) for x in (a, a, a, a, s, s, a, a, a, a)]

    def check(res):
        assert [int(r["state"][1]) for r in res] == [4, 4, 4, 0, 1, 1, 1, 0, 0, 0]
        assert [int(r["stats"][3]) for r in res] == [0, 0, 0, 1, 1, 0, 0, 0, 1, 1]
        assert [int(r["stats"][4]) for r in res] == [0, 0, 0, 0, 0, 1, 1, 1, 0, 0]
        assert [int(r["hold"][1]) for r in res] == [0, 0, 0, 0, 1, 2, 3, 0, 0, 0]
        assert [int(r["base_fill"][1]) for r in res][4:9] == [2, 2, 2, 2, 3]

    return Case("admission withheld while slow, resumed after the bit clears", _cfg(hold_max=100), steps, check)


def _fast_admitted() -> Case:
    a, s = win({1: {100: 20}}), win({1: {200: 20}})
    steps = [(x, 3) for x in (s, s, s, s, a, a, a, a)]

    def check(res):
        assert [int(r["state"][1]) for r in res] == [4, 4, 4, 0, 2, 2, 2, 2]
        assert [int(r["stats"][3]) for r in res] == [0, 0, 0, 1, 1, 1, 1, 1] and all(int(r["stats"][4]) == 0 for r in res)
        assert int(res[7]["fast_at"][1]) == 100 and int(res[7]["hold"][1]) == 0

    return Case("fast is admitted", _cfg(), steps, check)


def _rebase() -> Case:
    """hold_max = 3: slow at steps 4, 5, 6, so step 6 drops the baseline (two windows admitted so far, in ring
    rows 0 and 1, which stay as they are). Step 7 admits into row 2 beside the stale rows; by step 9 the ring is
    full again, every row rewritten, and step 10 gives up the oldest (step 7's admission). The slow windows
    hold 10 + i records, so the baseline's total names the windows it is made of."""
    a = win({1: {100: 20}})
    s = [win({1: {200: 10 + i}}) for i in range(8)]
    steps = [(x, 3) for x in [a, a, a, a] + s]

    def check(res):
        assert [int(r["state"][1]) for r in res][3:8] == [0, 1, 1, dr.WARMING | dr.REBASED, 0]
        assert [int(r["hold"][1]) for r in res][3:8] == [0, 1, 2, 0, 0] and int(res[6]["stats"][5]) == 1
        assert int(res[6]["n_base"][1]) == 40 and int(res[6]["base_fill"][1]) == 2   # the row it was decided on
        assert [int(r["base_fill"][1]) for r in res][7:] == [1, 2, 3, 3, 3]
        assert [int(r["n_base"][1]) for r in res][7:] == [10, 21, 33, 36, 39]

    return Case("hold_max reached: the rebase and the admissions after it", _cfg(crit=1.0), steps, check)


def _silent() -> Case:
    """Service 1 goes silent after the second step (its recent sample empties, its baseline stays), step 3 is
    empty, the group count changes between steps."""
    rng = np.random.default_rng(102)
    groups = [3, 3, 2, 3, 0, 1, 3, 3]
    steps = []
    for w, G in enumerate(groups):
        r = np.zeros(0, R.SPAN) if w == 3 else mixed_window(rng, 60, max(G, 1), [300.0, 500.0, 80.0])
        if w >= 2 and len(r):
            r = r[r["group_id"] != 1]
        steps.append((r, G))

    def check(res):
        assert int(res[1]["n_recent"][1]) > 20 and int(res[3]["n_recent"][1]) == 0 and int(res[3]["n_win"].sum()) == 0
        assert res[3]["q_recent"][1].tolist() == [EMPTY] * 4 and int(res[3]["state"][1]) == dr.WARMING
        assert int(res[7]["n_base"][1]) > 20 and int(res[7]["base_fill"][1]) == 2
        assert int(res[4]["stats"][2]) > 0 and int(res[4]["stats"][0]) == 0   # n_groups 0: everything out of group

    return Case("a service goes silent, n_groups changes", _cfg(), steps, check)


def _hot(buckets: int) -> Case:
    """4096 records of one service in one bucket, or over three adjacent ones, twice."""
    rng = np.random.default_rng(12 + buckets)
    b = 200 + rng.integers(0, buckets, 4096)
    r = recs([val(int(x), top=bool(j & 1)) for j, x in enumerate(b)], np.ones(4096, np.int64))

    def check(res):
        assert int(res[0]["n_win"][1]) == 4096 and int(res[1]["n_recent"][1]) == 8192
        assert 200 <= int(res[0]["q_recent"][1][0]) < 200 + buckets

    return Case(f"hot {'one bucket' if buckets == 1 else 'three buckets'}", _cfg(group_cap=2, span_cap=4096), [(r, 2), (r, 2)], check)


def _wide() -> Case:
    """8 services x 64 buckets: 512 keys into a table of 256 slots."""
    rng = np.random.default_rng(21)
    n = 3000
    r = recs([val(int(x)) for x in 150 + rng.integers(0, 64, n)], rng.integers(0, 8, n))

    def check(res):
        assert int(res[0]["n_win"].sum()) == n and int(res[1]["n_recent"].sum()) == 2 * n

    return Case("hot wide: more keys than the table holds", _cfg(group_cap=8, span_cap=4096), [(r, 8), (r[::-1], 8)], check)


def _random() -> Case:
    """18 steps of 5 services: service 0 calm, 1 shifts up by 40 % at step 8 and stays (withheld, then rebased),
    2 gets faster at step 8, 3 is sparse, 4 is present in some steps only."""
    rng = np.random.default_rng(13)
    steps = []
    for w in range(18):
        G = 5 if w % 5 else 4
        med = [300.0, 400.0 * (1.4 if w >= 8 else 1.0), 900.0 / (1.5 if w >= 8 else 1.0), 250.0, 120.0]
        r = mixed_window(rng, 3000 if w == 1 else int(rng.integers(150, 400)), G, med)
        keep = (r["group_id"] != 3) | (rng.random(len(r)) < 0.05)
        steps.append((r[keep], G))

    def check(res):
        states = np.array([r["state"] for r in res])
        assert (states[:8, :3] & (dr.SLOW | dr.FAST)).sum() == 0
        assert (states[8:, 1] & dr.SLOW).any() and (states[8:, 2] & dr.FAST).any() and (states[:, 1] & dr.REBASED).any()
        assert sum(int(r["stats"][4]) for r in res) > 0

    return Case("hot random 3000", _cfg(group_cap=5, span_cap=4096, min_recent=30, min_base=60, min_base_windows=2, hold_max=4),
                steps, check)


def cases() -> List[Case]:
    out = [_identical(), _disjoint()]
    out += [_max_at(k) for k in (6, 7, 349, 350, 0, 384)] + [_max_at(7, fast=True), _max_at(349, fast=True), _last_bucket()]
    out += [_tie(False), _tie(True), _crit_edge(False), _crit_edge(True)]
    out += [_shift(d, p90) for p90 in (False, True) for d in (1, 2, 3)]
    out += [_threshold(w, below) for w in ("min_recent", "min_base", "min_base_windows") for below in (False, True)]
    out += [_rings(), _empty_not_admitted(), _withheld(), _fast_admitted(), _rebase(), _silent()]
    out += [_hot(1), _hot(3), _wide(), _random()]
    return out


CASE_NAMES = [c.name for c in cases()]


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


def run_pipeline(engine: str, windows: List[np.ndarray], n_groups, drift: Optional[Tuple[int, int, int]], group_cap: int = 8, **kw):
    """The windows through ``WindowPipeline(engine, ttft_drift=drift)`` and a ``RingWindowSource`` over a
    span ring. Returns (per-window results, per-window tracker results (empty with ``drift`` = None))."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import Cut, RingWindowSource, WindowPipeline
    from llm_slo_ebpf_toolkit_amd.runtime import load

    rt = load()
    pipe = WindowPipeline(4096, 1024, group_cap, model="bayes", learn=False, user_cap=1024, engine=engine,
                          ttft_slo_ms=800.0, window_ms=160.0, ttft_drift=drift, **kw)
    ring = rt.HostRing(1 << 12, 64)
    src = RingWindowSource(pipe, None, None, ring)
    res, out = [], []
    try:
        for w, r in enumerate(windows):
            G = n_groups if np.isscalar(n_groups) else n_groups[w]
            assert ring.push(r) == len(r)
            kk = src.stage(Cut(kernel=0, user=0, spans=ring.head, t_ns=1_700_000_000_000_000_000 + w * 160_000_000), G)["k"]
            res.append({key: np.array(v, copy=True) for key, v in pipe.results(kk, G).items()})
            if drift:
                out.append({key: np.array(v, copy=True) for key, v in pipe.drift_results(kk, G).items()})
        src.drain()
    finally:
        pipe.close()
    return res, out


# configurations both classes must refuse (the wrap bound: 2^16 squared x 64 x 64 = 2^44)
BAD_CONFIGS = [dict(recent=0), dict(recent=1025), dict(gap=0), dict(gap=1025), dict(baseline=0), dict(baseline=4097),
               dict(group_cap=0), dict(group_cap=65537), dict(span_cap=0), dict(span_cap=1 << 16, recent=64, baseline=64),
               dict(span_cap=1 << 22, recent=1, baseline=1), dict(n_buffers=0), dict(n_buffers=65), dict(crit=0.0),
               dict(crit=-1.0), dict(crit=float("nan")), dict(crit=float("inf")), dict(min_shift=-1), dict(min_shift=386),
               dict(min_recent=0), dict(min_base=0), dict(min_base_windows=0), dict(hold_max=0),
               dict(group_cap=65536, baseline=4096)]
