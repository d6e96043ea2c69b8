"""Span windows for the error SLI tests (pipeline/errsli.py, ops/errsli.py): builders of windows, the named
cases both test files run (CASES), each with a hand-computed expectation, and the brute force the oracle is
checked against -- a plain Python loop over the records and a list of every step's counts, every window sum
recomputed from that list (never rolled), Python integers for the compare."""

from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.pipeline import errsli as es

OK, CLIENT, CANCELLED, THROTTLED, TIMEOUT, UNAVAILABLE, SERVER, OTHER = range(8)
# target 0.9: budget_ppm = 100000; with factor 1.0 (1000 milli) a window burns at bad / n >= 0.1
TARGET = 0.9
BUDGET = 100_000
F1 = 1000


def recs(cls: Sequence[int], grp: Sequence[int], flags=0, ttft=np.nan) -> np.ndarray:
    """Finished requests of the classes ``cls`` over the flag bits ``flags`` (a value or one per record)."""
    n = len(cls)
    r = np.zeros(n, dtype=R.SPAN)
    r["ttft_ms"] = np.asarray(ttft, dtype=np.float32)
    r["group_id"] = np.asarray(grp, dtype=np.uint32)
    r["flags"] = np.asarray(flags, dtype=np.uint32) | R.pack_outcome(np.asarray(cls, dtype=np.int64))
    r["ts_ns"] = 1_700_000_000_000_000_000 + np.arange(n)
    r["trace_h"] = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    r["latency_ms"] = 20.0
    return r


def of(g: int, **by_class: int) -> np.ndarray:
    """``of(0, ok=8, server=2)``: that many requests of service ``g`` per class."""
    cls = [es.CLASSES.index(k) for k, n in by_class.items() for _ in range(n)]
    return recs(cls, [g] * len(cls))


def cat(*parts: np.ndarray) -> np.ndarray:
    return np.concatenate(parts) if parts else np.zeros(0, R.SPAN)


def mixed_window(rng, n: int, G: int, p_bad: float = 0.15) -> np.ndarray:
    """About ``n`` finished requests of ``G`` services, mostly ok and each service with its own failing
    class, with SPAN_NO_SLI / SPAN_LATE / TPOT bits and a TTFT or none at random; plus what the rule leaves
    out or counts aside: start and first-token records (with class bits set), reserved classes, groups at
    and above ``G``."""
    g = rng.integers(0, max(G, 1), n)
    cls = np.where(rng.random(n) < p_bad, 1 + (g % 7), 0)
    fl = (np.where(rng.random(n) < 0.5, R.SPAN_NO_SLI, 0) | np.where(rng.random(n) < 0.1, R.SPAN_LATE, 0)
          | R.pack_tpot_us(rng.integers(0, 200_000, n)))
    ttft = np.where(rng.random(n) < 0.7, rng.lognormal(np.log(300.0), 1.0, n), np.nan)
    parts = [recs(cls, g, fl, ttft)]
    parts.append(recs([SERVER, 9, 15, OK], [G, G + 3, 0, G], 0))
    parts.append(recs([SERVER, TIMEOUT, 12], [0, 0, 0], [R.SPAN_FIRST_TOKEN, R.SPAN_START | R.SPAN_NO_SLI, R.SPAN_START]))
    out = np.concatenate(parts)
    return out[rng.permutation(len(out))]


# ---- the brute force ----------------------------------------------------------------------------
class Brute:
    """The rules record by record; ``hist`` holds every step's counts, and every sum is taken over its tail."""

    def __init__(self, group_cap: int, windows: int, target: float = TARGET, pairs=((2, 1, F1),), min_requests: int = 0,
                 bad_mask: int = es.BAD_DEFAULT, **_kw):
        self.C, self.W = group_cap, windows
        self.budget = min(10 ** 6, max(1, int((1.0 - target) * 1e6 + 0.5)))
        self.pairs, self.min_requests, self.bad_mask = [tuple(p) for p in pairs], min_requests, bad_mask
        self.hist: List[List[List[int]]] = []
        self.age = [0] * group_cap

    def _sum(self, g: int, last: int) -> Tuple[int, int]:
        n = bad = 0
        for step in self.hist[-last:]:
            for c, k in enumerate(step[g]):
                n += k
                if (self.bad_mask >> c) & 1:
                    bad += k
        return n, bad

    def step(self, records: np.ndarray, n_groups: int) -> Dict[str, np.ndarray]:
        stats = dict.fromkeys(es.STATS, 0)
        counts = [[0] * 8 for _ in range(self.C)]
        for r in records:
            fl = int(r["flags"])
            if fl & (R.SPAN_START | R.SPAN_FIRST_TOKEN):
                continue
            g, c = int(r["group_id"]), (fl >> 4) & 15
            if g >= n_groups:
                stats["out_of_group"] += 1
            elif c >= 8:
                stats["reserved"] += 1
            else:
                stats["observed"] += 1
                counts[g][c] += 1
        self.hist.append(counts)
        out = es.empty_result(self.C)
        for g in range(self.C):
            out["counts"][g] = counts[g]
            out["counts_roll"][g] = [sum(step[g][c] for step in self.hist[-self.W:]) for c in range(8)]
            fire = 0
            for p, (L, S, f) in enumerate(self.pairs):
                nl, bl = self._sum(g, L)
                ns, bs = self._sum(g, S)
                out["pair_sums"][g, p] = [nl, bl, ns, bs]
                thr = f * self.budget
                if all(n >= self.min_requests and n > 0 and b * 10 ** 9 >= thr * n for n, b in ((nl, bl), (ns, bs))):
                    fire |= 1 << p
            self.age[g] = min(self.age[g] + 1, 2 ** 32 - 1) if fire else 0
            out["firing"][g], out["age"][g] = fire, self.age[g]
        out["stats"][:len(es.STATS)] = [stats[name] for name in es.STATS]
        return out

    def resident(self) -> Dict[str, np.ndarray]:
        out = {"counts": np.zeros((self.C, 8), np.uint32), "pair_sums": np.zeros((self.C, 4, 4), np.uint32),
               "age": np.asarray(self.age, np.uint32), "pos": len(self.hist) % self.W}
        for g in range(self.C):
            out["counts"][g] = [sum(step[g][c] for step in self.hist[-self.W:]) for c in range(8)]
            for p, (L, S, _f) in enumerate(self.pairs):
                out["pair_sums"][g, p] = [*self._sum(g, L), *self._sum(g, S)]
        return out


def same_results(a: dict, b: dict, what: str = "") -> None:
    assert set(a) == set(b) == set(es.RESULT_FIELDS), what
    for f in es.RESULT_FIELDS:
        assert a[f].dtype == b[f].dtype == np.uint32 and a[f].shape == b[f].shape, (what, f, a[f].dtype, b[f].dtype,
                                                                                    a[f].shape, b[f].shape)
        np.testing.assert_array_equal(a[f], b[f], err_msg=f"{what} {f}")


def same_resident(a: dict, b: dict, what: str = "") -> None:
    assert int(a["pos"]) == int(b["pos"]), (what, a["pos"], b["pos"])
    for f in ("counts", "pair_sums", "age"):
        assert a[f].dtype == b[f].dtype == np.uint32 and a[f].shape == b[f].shape, (what, f)
        np.testing.assert_array_equal(a[f], b[f], err_msg=f"{what} resident {f}")


# ---- the named cases ----------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    cfg: dict
    steps: List[Tuple[np.ndarray, int]]                # (records, n_groups)
    check: Optional[Callable[[List[dict]], None]] = None   # over every step's results (all rows of group_cap)


def _cfg(group_cap=3, windows=2, span_cap=256, pairs=((2, 1, F1),), min_requests=0, bad_mask=es.BAD_DEFAULT, target=TARGET):
    return dict(group_cap=group_cap, windows=windows, span_cap=span_cap, target=target, pairs=[tuple(p) for p in pairs],
                min_requests=min_requests, bad_mask=bad_mask)


def _every_class() -> Case:
    r = recs(list(range(16)), [0] * 16)

    def check(res):
        assert res[0]["counts"][0].tolist() == [1] * 8 and res[0]["counts_roll"][0].tolist() == [1] * 8
        assert es.stats_dict(res[0]["stats"]) == {"observed": 8, "out_of_group": 0, "reserved": 8}
        # n = 8, bad = 5 (classes 3-7) in both windows of the pair; 5 / 8 >= 0.1 fires
        assert res[0]["pair_sums"][0, 0].tolist() == [8, 5, 8, 5] and res[0]["firing"].tolist() == [1, 0, 0]

    return Case("every class and the reserved ones", _cfg(), [(r, 1)], check)


def _check_order() -> Case:
    r = recs([9, 9, 9, THROTTLED, SERVER, OK], [7, 7, 0, 0, 7, 2],
             [R.SPAN_START | R.SPAN_NO_SLI, 0, 0, 0, R.SPAN_FIRST_TOKEN, 0])

    def check(res):
        # skipped (start), out_of_group before reserved, reserved, observed, skipped (first token), out_of_group
        assert es.stats_dict(res[0]["stats"]) == {"observed": 1, "out_of_group": 2, "reserved": 1}
        assert res[0]["counts"][0].tolist() == [0, 0, 0, 1, 0, 0, 0, 0] and int(res[0]["counts"].sum()) == 1

    return Case("check order", _cfg(), [(r, 2)], check)


def _other_bits() -> Case:
    fl = [0, R.SPAN_NO_SLI, R.SPAN_LATE, R.SPAN_NO_SLI | R.SPAN_LATE, int(R.pack_tpot_us(R.SPAN_TPOT_MAX)), 0xFFFFFFF3]
    r = recs([SERVER] * 6, [1] * 6, fl, [np.nan, 10.0, -1.0, np.inf, 900.0, np.nan])

    def check(res):
        # the last record's own bits 4-7 are all set: class 15, reserved
        assert res[0]["counts"][1].tolist() == [0, 0, 0, 0, 0, 0, 5, 0] and int(res[0]["stats"][2]) == 1

    return Case("NO_SLI, LATE, TPOT bits and the TTFT do not matter", _cfg(), [(r, 2)], check)


def _bad_mask(mask: int, bad: int) -> Case:
    r = cat(of(0, ok=4, client=1, cancelled=2, throttled=3, server=1))

    def check(res):
        assert res[0]["pair_sums"][0, 0].tolist() == [11, bad, 11, bad]

    return Case(f"bad_mask {mask:#x}", _cfg(bad_mask=mask), [(r, 1)], check)


def _horizon(W: int) -> Case:
    """Service 1 goes silent after the second step; step 3 is empty; the group count changes; by step W + 1
    every window with a record of service 1 has left the horizon and the pair's long window."""
    rng = np.random.default_rng(200 + W)
    groups = [3, 3, 2, 3, 0, 1, 3, 3]
    steps = []
    for w, G in enumerate(groups):
        r = np.zeros(0, R.SPAN) if w == 3 else mixed_window(rng, 60, max(G, 1))
        if w >= 2 and len(r):
            r = r[r["group_id"] != 1]
        steps.append((r, G))

    def check(res):
        assert int(res[1]["counts_roll"][1].sum()) > 20 and int(res[W + 1]["counts_roll"][1].sum()) == 0
        assert res[W + 1]["pair_sums"][1].tolist() == [[0] * 4] * 4
        assert int(res[3]["counts"].sum()) == 0 and int(res[3]["counts_roll"].sum()) > 0
        assert int(res[4]["stats"][0]) == 0 and int(res[4]["stats"][1]) > 0  # n_groups = 0: everything out of group

    return Case(f"horizon W={W}", _cfg(windows=W, pairs=((W, 1, F1),)), steps, check)


def _both_windows() -> Case:
    """L = 3 = W, S = 1, factor 1 at a 10 % budget. Hand-computed (n_long, bad_long, n_short, bad_short):
      0: 10 ok                 (10, 0, 10, 0)   neither burns
      1: 8 ok + 2 server       (20, 2, 10, 2)   long 2/20 = 0.1 exactly, short 0.2: fires
      2: 10 ok                 (30, 2, 10, 0)   neither
      3: 5 ok + 5 server       (30, 7, 10, 5)   step 0 left the long window (L == W): fires
      4: 10 ok                 (30, 5, 10, 0)   the long window still burns, the short does not: no fire
      5: 100 ok                (120, 5, 100, 0) neither
      6: 9 ok + 1 timeout      (120, 1, 10, 1)  the short window burns (0.1 exactly), the long does not: no fire"""
    steps = [of(0, ok=10), of(0, ok=8, server=2), of(0, ok=10), of(0, ok=5, server=5), of(0, ok=10), of(0, ok=100),
             of(0, ok=9, timeout=1)]

    def check(res):
        assert [r["pair_sums"][0, 0].tolist() for r in res] == [[10, 0, 10, 0], [20, 2, 10, 2], [30, 2, 10, 0], [30, 7, 10, 5],
                                                               [30, 5, 10, 0], [120, 5, 100, 0], [120, 1, 10, 1]]
        assert [int(r["firing"][0]) for r in res] == [0, 1, 0, 1, 0, 0, 0]
        assert [int(r["age"][0]) for r in res] == [0, 1, 0, 1, 0, 0, 0]
        assert res[6]["counts_roll"][0].tolist() == [119, 0, 0, 0, 1, 0, 0, 0]

    return Case("a pair fires only when both windows burn, L == W", _cfg(windows=3, pairs=((3, 1, F1),)),
                [(s, 1) for s in steps], check)


def _equality() -> Case:
    """bad / n >= 0.1: 1 of 10 burns (equality), 1 of 11 does not, 1 of 9 does."""
    r = cat(of(0, ok=9, other=1), of(1, ok=10, other=1), of(2, ok=8, other=1))

    def check(res):
        assert res[0]["firing"].tolist() == [1, 0, 1] and res[0]["pair_sums"][:, 0, 0].tolist() == [10, 11, 9]

    return Case("the compare at equality and one request either side", _cfg(windows=1, pairs=((1, 1, F1),)), [(r, 3)], check)


def _min_requests() -> Case:
    r = cat(of(0, unavailable=10), of(1, unavailable=9), of(2, ok=10))

    def check(res):
        assert res[0]["firing"].tolist() == [1, 0, 0] and res[0]["age"].tolist() == [1, 0, 0]

    return Case("min_requests either side", _cfg(windows=1, pairs=((1, 1, F1),), min_requests=10), [(r, 3)], check)


def _no_requests() -> Case:
    """min_requests = 0 and nothing at all: 0 * 10^9 >= thr * 0 holds, n > 0 does not."""
    def check(res):
        assert [r["firing"].tolist() for r in res] == [[0, 0, 0]] * 2 and int(res[1]["counts_roll"].sum()) == 0

    return Case("n = 0 never burns", _cfg(), [(np.zeros(0, R.SPAN), 3), (of(2, ok=1)[:0], 3)], check)


def _age() -> Case:
    bad, good = of(1, server=3), of(1, ok=3)
    steps = [bad, bad, bad, good, bad, bad, np.zeros(0, R.SPAN), bad]

    def check(res):
        assert [int(r["age"][1]) for r in res] == [1, 2, 3, 0, 1, 2, 0, 1]
        assert [int(r["age"][0]) for r in res] == [0] * 8

    return Case("age counts up, resets and resumes", _cfg(windows=2, pairs=((1, 1, F1),)), [(s, 2) for s in steps], check)


def _four_pairs() -> Case:
    """W = 4, pairs (4,2) (3,3) (2,1) (1,1) at factors 1, 2, 5, 10 (bad / n >= 0.1, 0.2, 0.5, 1.0).
      0: 10 ok            all zero bad                                          firing 0
      1: 5 ok + 5 server  p0 (20,5,20,5) p1 (20,5,20,5) p2 (20,5,10,5) p3 (10,5,10,5)
                          p0 0.25/0.25 fires; p1 0.25 >= 0.2 fires; p2 long 0.25 < 0.5 no; p3 0.5 < 1 no: 0b0011
      2: 10 server        p0 (30,15,20,15) p1 (30,15,30,15) p2 (20,15,10,10) p3 (10,10,10,10): all fire, 0b1111
      3: 10 ok            p0 (40,15,20,10) p1 (30,15,30,15) p2 (20,10,10,0) p3 (10,0,10,0): 0b0011
      4: 10 ok            step 0 left p0's long window: p0 (40,15,20,0) short 0 no; p1 (30,10,30,10) 0.33 fires: 0b0010"""
    steps = [of(0, ok=10), of(0, ok=5, server=5), of(0, server=10), of(0, ok=10), of(0, ok=10)]
    pairs = ((4, 2, 1000), (3, 3, 2000), (2, 1, 5000), (1, 1, 10000))

    def check(res):
        assert [int(r["firing"][0]) for r in res] == [0, 0b0011, 0b1111, 0b0011, 0b0010]
        assert res[2]["pair_sums"][0].tolist() == [[30, 15, 20, 15], [30, 15, 30, 15], [20, 15, 10, 10], [10, 10, 10, 10]]
        assert res[4]["pair_sums"][0].tolist() == [[40, 15, 20, 0], [30, 10, 30, 10], [20, 0, 10, 0], [10, 0, 10, 0]]
        assert [int(r["age"][0]) for r in res] == [0, 1, 2, 3, 4]

    return Case("four pairs", _cfg(windows=4, pairs=pairs), [(s, 1) for s in steps], check)


def _fewer_steps() -> Case:
    """L = S = 3 in a horizon of 5: the first two steps sum what there is."""
    steps = [of(0, ok=1, server=1), of(0, ok=2), of(0, ok=3), of(0, ok=4)]

    def check(res):
        assert [r["pair_sums"][0, 0].tolist() for r in res] == [[2, 1, 2, 1], [4, 1, 4, 1], [7, 1, 7, 1], [9, 0, 9, 0]]
        assert [int(r["firing"][0]) for r in res] == [1, 1, 1, 0]

    return Case("fewer steps than L", _cfg(windows=5, pairs=((3, 3, F1),)), [(s, 1) for s in steps], check)


def _hot_one_key() -> Case:
    r = recs([SERVER] * 16383, [1] * 16383)

    def check(res):
        assert res[0]["counts"][1].tolist() == [0, 0, 0, 0, 0, 0, 16383, 0] and int(res[0]["stats"][0]) == 16383

    return Case("hot one key, 16383 records", _cfg(group_cap=2, span_cap=16384), [(r, 2)], check)


def _hot_wide() -> Case:
    """256 records, one workgroup, every record its own key out of 40 services x 8 classes: 256 keys hashed
    into 256 slots with 8 probes, so some find no slot and go to the row themselves."""
    i = np.arange(256)
    r = recs((i // 40) % 8, i % 40)

    def check(res):
        assert int(res[0]["counts"].sum()) == 256 and int((res[0]["counts"] == 1).sum()) == 256
        assert int(res[1]["counts_roll"].sum()) == 512

    return Case("hot wide: 40 services x 8 classes in one workgroup", _cfg(group_cap=40), [(r, 40), (r[::-1].copy(), 40)], check)


def _hot_257() -> Case:
    r = recs([OK] * 256 + [TIMEOUT], [0] * 256 + [2])

    def check(res):
        assert res[0]["counts"][0, 0] == 256 and res[0]["counts"][2, TIMEOUT] == 1

    return Case("hot 257: the second workgroup's flush", _cfg(span_cap=512), [(r, 3)], check)


def _hot_random() -> Case:
    rng = np.random.default_rng(17)
    steps = []
    for w in range(12):
        G = int(rng.integers(1, 6))
        steps.append((mixed_window(rng, 3000 if w == 1 else int(rng.integers(0, 300)), G, p_bad=float(rng.random()) * 0.3), G))
    return Case("hot random 12 steps", _cfg(group_cap=5, windows=4, span_cap=4096, pairs=((4, 1, F1), (3, 2, 2000), (2, 2, 500)),
                                            min_requests=20), steps)


def cases() -> List[Case]:
    return [_every_class(), _check_order(), _other_bits(), _bad_mask(0xF8, 4), _bad_mask(0xFE, 7), _bad_mask(0x08, 3),
            _horizon(2), _horizon(3), _both_windows(), _equality(), _min_requests(), _no_requests(), _age(), _four_pairs(),
            _fewer_steps(), _hot_one_key(), _hot_wide(), _hot_257(), _hot_random()]


CASE_NAMES = [c.name for c in cases()]


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


# every configuration check, one violation each (the rest at the defaults or small)
_P = [(1, 1, F1)]
BAD_CONFIGS = [dict(windows=0, pairs=_P), dict(windows=32769, pairs=_P), dict(group_cap=0), dict(group_cap=65537), dict(span_cap=0),
               dict(n_buffers=0), dict(n_buffers=65), dict(target=1.0), dict(target=-0.1), dict(target=float("nan")),
               dict(target=float("inf")), dict(pairs=[]), dict(pairs=_P * 5), dict(windows=4, pairs=[(5, 1, F1)]),
               dict(windows=4, pairs=[(2, 3, F1)]), dict(windows=4, pairs=[(2, 0, F1)]), dict(windows=4, pairs=[(2, 1, 0)]),
               dict(windows=4, pairs=[(2, 1, 10001)], target=0.9),  # 10001 * 100000 > 10^9
               dict(min_requests=-1), dict(min_requests=1 << 32), dict(bad_mask=0), dict(bad_mask=0xF9), dict(bad_mask=0x1F8),
               dict(span_cap=1 << 21, windows=2048, pairs=_P),        # span_cap * windows = 2^32
               dict(group_cap=65536, windows=32768, pairs=_P)]        # far beyond 2 GiB
GOOD_CONFIGS = [dict(windows=1, group_cap=1, span_cap=1, n_buffers=1, target=0.0, pairs=[(1, 1, 1)], min_requests=0, bad_mask=2),
                dict(windows=32768, group_cap=64, pairs=[(32768, 32768, F1)]),
                dict(windows=4, pairs=[(2, 1, 10000)], target=0.9)]   # the product exactly 10^9

PIPE_PAIRS = ((2, 1, F1), (2, 2, 2000))


def run_pipeline(engine: str, windows: List[np.ndarray], n_groups, horizon: int, group_cap: int = 8, **kw):
    """The windows through ``WindowPipeline(engine, error_sli=horizon)`` and a ``RingWindowSource`` over a
    span ring. Returns (per-window results, per-window tracker results (empty with ``horizon`` = 0))."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import Cut, RingWindowSource, WindowPipeline
    from llm_slo_ebpf_toolkit_amd.runtime import load

    rt = load()
    if horizon:
        kw = dict(error_sli=horizon, error_target=TARGET, error_pairs=PIPE_PAIRS, error_min_requests=5, **kw)
    pipe = WindowPipeline(4096, 1024, group_cap, model="bayes", learn=False, user_cap=1024, engine=engine,
                          ttft_slo_ms=800.0, window_ms=160.0, **kw)
    ring = rt.HostRing(1 << 12, 64)
    src = RingWindowSource(pipe, None, None, ring)
    res, err = [], []
    try:
        for w, r in enumerate(windows):
            G = n_groups if np.isscalar(n_groups) else n_groups[w]
            assert ring.push(r) == len(r)
            kk = src.stage(Cut(kernel=0, user=0, spans=ring.head, t_ns=1_700_000_000_000_000_000 + w * 160_000_000), G)["k"]
            res.append({key: np.array(v, copy=True) for key, v in pipe.results(kk, G).items()})
            if horizon:
                err.append({key: np.array(v, copy=True) for key, v in pipe.error_results(kk, G).items()})
        src.drain()
    finally:
        pipe.close()
    return res, err
