"""Span windows for the pod-breakdown tests (pipeline/podrank.py, ops/podrank.py): seeded windows with
pods, the rule's edge values, colliding pods, and the brute force the oracle is checked against (a
plain dict of dicts over the counted records, no keys, no numpy reductions)."""

import math
import struct
from typing import Dict, List, Sequence

import numpy as np

from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.pipeline import podrank as pr
from tests.slisketch_scenarios import spans, window  # noqa: F401  (reused, not edited)

F32 = np.float32
SLO = 800.0
# equal to the SLO (no breach), just above it (a breach), +inf (a breach), -0.0 (counted, ranks as 0), NaN and -1
# (invalid), and values around the sum's clamp
EDGE_TTFT = [F32(800.0), np.nextafter(F32(800), F32(np.inf)), F32(np.inf), F32(-0.0), F32(0.0), F32(np.nan), F32(-1.0),
             F32(2 ** 21), F32(3e6), F32(1e-40), F32(437.5)]
# the unknown pod, the largest pod with a row, the first without
EDGE_PODS = [0, (1 << 20) - 1, 1 << 20, 0xFFFFFFFF, 7]


def with_pods(recs: np.ndarray, pods) -> np.ndarray:
    recs = recs.copy()
    recs["pod_id"] = np.asarray(pods, dtype=np.uint32)
    return recs


def pod_spans(ttft: Sequence[float], grp: Sequence[int], pods: Sequence[int], flags=R.SPAN_FIRST_TOKEN) -> np.ndarray:
    return with_pods(spans(ttft, grp, flags), pods)


def edge_window(rng, n: int, G: int, n_pods: int = 12) -> np.ndarray:
    """About ``n`` log-normal records over ``G`` groups and ``n_pods`` pods, plus every edge TTFT on a
    small pod and every edge pod with a value on each side of the SLO, in every group, SPAN_LATE on
    some, and what the rule skips (SPAN_NO_SLI, start records, groups at and above ``G``)."""
    base = window(rng, n, G, G, edges=False)
    parts = [with_pods(base, rng.integers(1, n_pods + 1, len(base)))]
    for g in range(G):
        e = pod_spans(EDGE_TTFT, [g] * len(EDGE_TTFT), rng.integers(1, 4, len(EDGE_TTFT)))
        e["flags"][::3] |= R.SPAN_LATE
        parts.append(e)
        parts.append(pod_spans([100.0, 900.0] * len(EDGE_PODS), [g] * (2 * len(EDGE_PODS)), np.repeat(EDGE_PODS, 2)))
    parts.append(pod_spans([900.0, 50.0], [G, G + 3], [1, 2]))
    out = np.concatenate(parts)
    return out[rng.permutation(len(out))]


def colliding_pods(g: int, slots: int, want_slot: int, count: int, start: int = 1) -> List[int]:
    """``count`` pods whose pair (g, pod) hashes to ``want_slot`` in a table of ``slots``."""
    out, pod = [], start
    while len(out) < count:
        if pr.slot_of(g, pod, slots) == want_slot:
            out.append(pod)
        pod += 1
        assert pod < pr.POD_LIMIT
    return out


def _bits(v) -> int:
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def brute_pairs(w: np.ndarray, n_groups: int, slo: float = SLO):
    """(totals {g: [n, b]}, pairs {g: {pod: [n, b, max_bits, sum_milli]}}, stats by name) of one
    window, record by record in plain Python."""
    tot: Dict[int, List[int]] = {}
    pairs: Dict[int, Dict[int, List[int]]] = {}
    stats = dict.fromkeys(pr.STATS, 0)
    slo32 = float(F32(slo))
    for r in w:
        if int(r["flags"]) & R.SPAN_NO_SLI:
            continue
        g, v, pod = int(r["group_id"]), float(r["ttft_ms"]), int(r["pod_id"])
        if g >= n_groups:
            stats["out_of_group"] += 1
            continue
        if not v >= 0.0:
            stats["invalid"] += 1
            continue
        stats["observed"] += 1
        breach = int(v > slo32)
        t = tot.setdefault(g, [0, 0])
        t[0] += 1
        t[1] += breach
        if pod >= 1 << 20:
            stats["pod_out_of_range"] += 1
            continue
        p = pairs.setdefault(g, {}).setdefault(pod, [0, 0, 0, 0])
        p[0] += 1
        p[1] += breach
        p[2] = max(p[2], _bits(v) & 0x7FFFFFFF)
        milli = float(min(v, 2.0 ** 21)) * 1000.0
        p[3] += int(round(milli)) if math.isfinite(milli) else 0  # round half to even, like rint
    return tot, pairs, stats


def brute_merge(history: Sequence[dict]) -> dict:
    """The pairs of several windows (``brute_pairs``' second value each) under one key each."""
    out: Dict[int, Dict[int, List[int]]] = {}
    for pairs in history:
        for g, pods in pairs.items():
            for pod, (n, b, mx, sm) in pods.items():
                p = out.setdefault(g, {}).setdefault(pod, [0, 0, 0, 0])
                p[0] += n
                p[1] += b
                p[2] = max(p[2], mx)
                p[3] += sm
    return out


def brute_scope(pairs: dict, group_cap: int, k: int) -> Dict[str, np.ndarray]:
    """pods / pods_b / k_top / top of ``pairs`` by a plain sort: breaches descending, requests
    ascending, pod ascending."""
    res = {"pods": np.zeros(group_cap, np.uint32), "pods_b": np.zeros(group_cap, np.uint32),
           "k_top": np.zeros(group_cap, np.uint32), "top": np.zeros((group_cap, k), pr.POD_ROW)}
    for g, pods in pairs.items():
        res["pods"][g] = len(pods)
        hot = sorted(((-b, n, pod) for pod, (n, b, _mx, _sm) in pods.items() if b >= 1))
        res["pods_b"][g] = len(hot)
        res["k_top"][g] = min(k, len(hot))
        for j, (_nb, _n, pod) in enumerate(hot[:k]):
            n, b, mx, sm = pods[pod]
            row = res["top"][g, j]
            row["pod_id"], row["n"], row["b"], row["sum_milli"] = pod, n, b, sm
            row["max_ttft"] = np.array([mx], np.uint32).view(F32)[0]
    return res


def brute_results(history_tot: Sequence[dict], history_pairs: Sequence[dict], stats: dict, group_cap: int, k: int,
                  windows: int) -> Dict[str, np.ndarray]:
    """A step's whole result from the brute-force windows so far (the newest last)."""
    res: Dict[str, np.ndarray] = {}
    for s, tots, pairs in (("win", history_tot[-1:], history_pairs[-1]),
                           ("rec", history_tot[-windows:], brute_merge(history_pairs[-windows:]))):
        n, b = np.zeros(group_cap, np.uint32), np.zeros(group_cap, np.uint32)
        for t in tots:
            for g, (tn, tb) in t.items():
                n[g] += tn
                b[g] += tb
        res[f"{s}_n"], res[f"{s}_b"] = n, b
        for f, a in brute_scope(pairs, group_cap, k).items():
            res[f"{s}_{f}"] = a
    st = np.zeros(pr.N_STATS, np.uint32)
    st[:len(pr.STATS)] = [stats[name] for name in pr.STATS]
    res["stats"] = st
    return res


def pairs_array(pairs: dict) -> np.ndarray:
    """``brute_pairs``' pairs as a PAIR list sorted by (g, pod)."""
    rows = [(g, pod, n, b, mx, sm) for g, pods in pairs.items() for pod, (n, b, mx, sm) in pods.items()]
    return pr.sort_pairs(np.array(rows, dtype=pr.PAIR) if rows else np.zeros(0, pr.PAIR))


def same_rows(a: np.ndarray, b: np.ndarray, what: str = "") -> None:
    """Rows compared as bytes."""
    assert a.dtype == b.dtype == pr.POD_ROW and a.shape == b.shape, (what, a.dtype, a.shape, b.shape)
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8),
                                  err_msg=what)


def same_results(a: dict, b: dict, what: str = "", G: int = None) -> None:
    """Every result array equal; ``G``: compare the first G rows of the per-group arrays only."""
    assert set(a) == set(b) == set(pr.RESULT_FIELDS), what
    for key in pr.RESULT_FIELDS:
        x, y = a[key], b[key]
        if G is not None and key != "stats":
            x, y = x[:G], y[:G]
        if key in ("win_top", "rec_top"):
            same_rows(x, y, f"{what} {key}")
        else:
            assert x.dtype == y.dtype and x.shape == y.shape, (what, key, x.dtype, y.dtype, x.shape, y.shape)
            np.testing.assert_array_equal(x, y, err_msg=f"{what} {key}")


def same_resident(a: Sequence[np.ndarray], b: Sequence[np.ndarray], what: str = "") -> None:
    """The horizon's lists, each sorted by (g, pod)."""
    assert len(a) == len(b), what
    for h, (x, y) in enumerate(zip(a, b)):
        x, y = pr.sort_pairs(np.asarray(x)), pr.sort_pairs(np.asarray(y))
        assert x.dtype == y.dtype == pr.PAIR and x.shape == y.shape, (what, h, x.shape, y.shape)
        assert x.tobytes() == y.tobytes(), f"{what} list {h}\n{x}\n{y}"


def overflow_invariants(res: dict, truth_pairs: dict, truth_tot: dict, lists_cur: np.ndarray, pair_cap: int,
                        what: str = "") -> None:
    """Past the capacity: exact totals, every kept pair's counts at most the truth, and the kept
    rows' requests plus the overflowed and the out-of-range records are the observed ones."""
    stats = pr.stats_dict(res["stats"])
    assert stats["pair_overflow"] > 0, what
    for g, (n, b) in truth_tot.items():
        assert int(res["win_n"][g]) == n and int(res["win_b"][g]) == b, (what, g)
    assert len(lists_cur) <= pair_cap, what
    for p in lists_cur:
        n, b, mx, sm = truth_pairs[int(p["g"])][int(p["pod"])]
        assert int(p["n"]) <= n and int(p["b"]) <= b and int(p["max_bits"]) <= mx and int(p["sum_milli"]) <= sm, (what, p)
    assert int(lists_cur["n"].sum()) + stats["pair_overflow"] + stats["pod_out_of_range"] == stats["observed"], what
    assert int(res["win_pods"].sum()) == len(lists_cur), what
    for g in range(len(res["win_k_top"])):
        for row in res["win_top"][g][:int(res["win_k_top"][g])]:
            n, b, _mx, _sm = truth_pairs[g][int(row["pod_id"])]
            assert 1 <= int(row["b"]) <= b and int(row["n"]) <= n, (what, g, row)


def run_pipeline(engine: str, windows: List[np.ndarray], n_groups, k: int, horizon: int = 3, group_cap: int = 8,
                 pairs: int = 256):
    """The windows through ``WindowPipeline(engine, pod_breakdown=k)`` and a ``RingWindowSource``
    over a span ring. Returns (per-window results, per-window tracker results; the latter empty
    with ``k`` = 0)."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import Cut, RingWindowSource, WindowPipeline
    from llm_slo_ebpf_toolkit_amd.runtime import load

    rt = load()
    pipe = WindowPipeline(4096, 1024, group_cap, model="bayes", learn=False, user_cap=1024, engine=engine,
                          ttft_slo_ms=SLO, window_ms=1000.0, pod_breakdown=k, pod_windows=horizon, pod_pairs=pairs)
    ring = rt.HostRing(1 << 12, 64)
    src = RingWindowSource(pipe, None, None, ring)
    res, pods = [], []
    try:
        for w, recs in enumerate(windows):
            G = n_groups if np.isscalar(n_groups) else n_groups[w]
            assert ring.push(recs) == len(recs)
            kk = src.stage(Cut(kernel=0, user=0, spans=ring.head), G)["k"]
            res.append({key: np.array(v, copy=True) for key, v in pipe.results(kk, G).items()})
            if k:
                pods.append({key: np.array(v, copy=True) for key, v in pipe.pod_results(kk, G).items()})
        src.drain()
    finally:
        pipe.close()
    return res, pods
