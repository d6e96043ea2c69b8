"""Span windows for the TTFT sketch's tests (pipeline/slisketch.py, ops/slisketch.py): seeded
log-normal TTFTs with the rule's edge values mixed in, and the brute-force statistics they are
checked against (sorted arrays and direct compares, no histogram)."""

from typing import List, Sequence

import numpy as np

from llm_slo_ebpf_toolkit_amd.collector import records as R

F32 = np.float32
INF = F32(np.inf)
MAX_MS = F32(2 ** 21)


def _next(v, to):
    return np.nextafter(F32(v), F32(to))


# (value, where the rule puts it): "under" / "over" = the underflow / overflow bucket, "in" = buckets
# 1..384, "invalid" = counted by the engine, in no histogram
EDGE_VALUES = [
    (F32(0.0), "under"), (F32(-0.0), "under"), (F32(1e-40), "under"), (_next(0.125, 0), "under"),
    (F32(0.125), "in"), (_next(0.125, 1), "in"), (_next(800, 0), "in"), (F32(800.0), "in"), (_next(800, INF), "in"),
    (_next(MAX_MS, 0), "in"), (MAX_MS, "over"), (_next(MAX_MS, INF), "over"), (INF, "over"),
    (F32(np.nan), "invalid"), (F32(-1.0), "invalid"),
]


def spans(ttft: Sequence[float], grp: Sequence[int], flags=R.SPAN_FIRST_TOKEN) -> np.ndarray:
    n = len(ttft)
    r = np.zeros(n, dtype=R.SPAN)
    r["ttft_ms"] = np.asarray(ttft, dtype=F32)
    r["group_id"] = np.asarray(grp, dtype=np.uint32)
    r["flags"] = flags
    r["ts_ns"] = 1_700_000_000_000_000_000 + np.arange(n)
    r["trace_h"] = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    r["latency_ms"] = np.where(np.isfinite(r["ttft_ms"]), r["ttft_ms"], 0)
    return r


def window(rng, n: int, n_groups: int, group_cap: int, edges: bool = True, skipped: bool = True) -> np.ndarray:
    """``n`` log-normal records (median ~300 ms, a heavy tail) over ``n_groups`` groups; with
    ``edges`` every edge value once, in random groups, SPAN_LATE on some; with ``skipped`` records the
    rule leaves out: SPAN_NO_SLI request spans, start records, groups at and above ``n_groups``."""
    parts = []
    if n and n_groups:
        parts.append(spans(rng.lognormal(np.log(300.0), 1.5, n), rng.integers(0, n_groups, n)))
    if edges and n_groups:
        e = spans([v for v, _ in EDGE_VALUES], rng.integers(0, n_groups, len(EDGE_VALUES)))
        e["flags"][::3] |= R.SPAN_LATE
        parts.append(e)
    if skipped:
        parts.append(spans([120.0, 900.0], [0, 0], R.SPAN_NO_SLI))
        parts.append(spans([np.nan], [0], R.SPAN_START | R.SPAN_NO_SLI))
        parts.append(spans([75.0, 3000.0], [n_groups, group_cap + 7]))
    if not parts:
        return np.zeros(0, R.SPAN)
    out = np.concatenate(parts)
    return out[rng.permutation(len(out))]


def counted(w: np.ndarray, n_groups: int):
    """(group, ttft) of the records the sketch observes, (engine-counted, invalid, out of group) counts."""
    sli = (w["flags"] & np.uint32(R.SPAN_NO_SLI)) == 0
    inside = sli & (w["group_id"] < n_groups)
    with np.errstate(invalid="ignore"):
        ok = inside & (w["ttft_ms"] >= 0)
    return w["group_id"][ok].astype(np.int64), w["ttft_ms"][ok], int(inside.sum()), int((inside & ~ok).sum()), \
        int((sli & ~inside).sum())


def brute_hist(grp: np.ndarray, v: np.ndarray, group_cap: int) -> np.ndarray:
    from llm_slo_ebpf_toolkit_amd.pipeline.slisketch import K, bucket_of

    h = np.zeros((group_cap, K), np.int64)
    for g in range(group_cap):
        h[g] = np.bincount(bucket_of(v[grp == g]), minlength=K)
    return h


def run_pipeline(engine: str, windows, n_groups, horizon: int, open_requests: int = 0, group_cap: int = 8):
    """The windows through ``WindowPipeline(engine, sli_sketch=horizon)`` and a ``RingWindowSource``
    over a span ring (cuts without a time: the sketch steps on every window). ``n_groups``: one
    number, or one per window. Returns (per-window results, per-window sketch results)."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import Cut, RingWindowSource, WindowPipeline
    from llm_slo_ebpf_toolkit_amd.runtime import load

    rt = load()
    pipe = WindowPipeline(4096, 1024, group_cap, model="bayes", learn=False, user_cap=1024, engine=engine,
                          ttft_slo_ms=800.0, window_ms=1000.0, open_requests=open_requests, sli_sketch=horizon)
    ring = rt.HostRing(1 << 12, 64)
    src = RingWindowSource(pipe, None, None, ring)
    res, sk = [], []
    try:
        for w, recs in enumerate(windows):
            G = n_groups if np.isscalar(n_groups) else n_groups[w]
            assert ring.push(recs) == len(recs)
            k = src.stage(Cut(kernel=0, user=0, spans=ring.head), G)["k"]
            res.append({key: np.array(v, copy=True) for key, v in pipe.results(k, G).items()})
            if horizon:
                sk.append({key: np.array(v, copy=True) for key, v in pipe.sli_results(k, G).items()})
        src.drain()
    finally:
        pipe.close()
    return res, sk


def exact_quantiles(v: np.ndarray) -> List[float]:
    """The nearest-rank values of the sorted array (rank r -> element r - 1) for the sketch's per-mille list."""
    from llm_slo_ebpf_toolkit_amd.pipeline.slisketch import PERMILLE

    s = np.sort(v.astype(np.float64))
    n = len(s)
    return [float(s[max(1, (q * n + 999) // 1000) - 1]) for q in PERMILLE]
