"""Span windows for the request-exemplar tests (pipeline/exemplars.py, ops/exemplars.py): the TTFT
sketch's seeded windows with identities filled in, the rule's edge values, and the brute force the
oracle is checked against (a plain ``np.lexsort`` over the counted records, no keys)."""

from typing import List, Sequence

import numpy as np

from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.pipeline import exemplars as ex
from tests.slisketch_scenarios import spans, window  # noqa: F401  (reused, not edited)

F32 = np.float32
# the order's edge values: -0.0 ranks with 0.0, +inf is first, NaN and -1 are invalid
EDGE_TTFT = [F32(0.0), F32(-0.0), F32(1e-40), F32(437.5), F32(437.5), F32(800.0), np.nextafter(F32(800), F32(np.inf)),
             F32(2 ** 21), F32(np.inf), F32(np.nan), F32(-1.0)]


def identify(recs: np.ndarray, rng) -> np.ndarray:
    """The records with span ids, latencies, retrieval times, pods and pids of their own."""
    n = len(recs)
    recs = recs.copy()
    recs["span_h"] = rng.integers(1, 1 << 63, n, dtype=np.uint64)
    recs["retr_ms"] = rng.uniform(0, 50, n).astype(F32)
    recs["pod_id"] = rng.integers(1, 40, n)
    recs["pid"] = rng.integers(100, 60000, n)
    return recs


def edge_window(rng, n: int, G: int) -> np.ndarray:
    """``n`` log-normal records over ``G`` groups plus every edge value in every group, SPAN_LATE on
    some, and what the rule skips (SPAN_NO_SLI, start records, groups at and above ``G``)."""
    parts = [window(rng, n, G, G, edges=False)]
    for g in range(G):
        e = spans(EDGE_TTFT, [g] * len(EDGE_TTFT))
        e["flags"][::3] |= R.SPAN_LATE
        parts.append(e)
    out = np.concatenate(parts)
    return identify(out[rng.permutation(len(out))], rng)


def counted(w: np.ndarray, n_groups: int) -> np.ndarray:
    """Indices of the records the tracker observes."""
    sli = (w["flags"] & np.uint32(R.SPAN_NO_SLI)) == 0
    with np.errstate(invalid="ignore"):
        return np.nonzero(sli & (w["group_id"] < n_groups) & (w["ttft_ms"] >= 0))[0]


def brute_window(w: np.ndarray, n_groups: int, group_cap: int, k: int):
    """(n [C], rows [C, k]) by lexsort: TTFT descending (as float64 magnitudes, -0.0 = 0.0), then index."""
    at = counted(w, n_groups)
    n = np.zeros(group_cap, np.uint32)
    rows = np.zeros((group_cap, k), ex.EXEMPLAR)
    for g in range(n_groups):
        a = at[w["group_id"][at] == g]
        n[g] = len(a)
        v = np.abs(w["ttft_ms"][a].astype(np.float64))
        a = a[np.lexsort((a, -v))][:k]
        rows[g, :len(a)] = ex.rows_of(w, a)
    return n, rows


def brute_recent(history: Sequence[np.ndarray], group_cap: int, k: int, windows: int):
    """(k_recent [C], rows [C, k]) from the last ``windows`` entries of ``history``, each a window's
    (rows [C, k], valid rows [C]) with ``history[-1]`` the newest: larger TTFT, then the newer window,
    then the earlier position."""
    last = list(history)[-windows:]
    out = np.zeros((group_cap, k), ex.EXEMPLAR)
    cnt = np.zeros(group_cap, np.uint32)
    for g in range(group_cap):
        cand = []
        for age, (rows, have) in enumerate(reversed(last)):
            for p in range(int(have[g])):
                cand.append((rows[g, p], age, p))
        if not cand:
            continue
        v = np.array([abs(float(r["ttft_ms"])) for r, _a, _p in cand])
        order = np.lexsort(([p for _r, _a, p in cand], [a for _r, a, _p in cand], -v))[:k]
        for j, c in enumerate(order):
            out[g, j] = cand[c][0]
            out[g, j]["age"] = cand[c][1]
        cnt[g] = len(order)
    return cnt, out


def same_rows(a: np.ndarray, b: np.ndarray, what: str = "") -> None:
    """Rows compared as bytes: NaN latencies and -0.0 included."""
    assert a.dtype == b.dtype == ex.EXEMPLAR and a.shape == b.shape, (what, a.dtype, a.shape, b.shape)
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8),
                                  err_msg=what)


def same_results(a: dict, b: dict, what: str = "") -> None:
    assert set(a) == set(b) == set(ex.RESULT_FIELDS), what
    for key in ex.RESULT_FIELDS:
        if key in ("win", "recent"):
            same_rows(a[key], b[key], f"{what} {key}")
        else:
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, (what, key)
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"{what} {key}")


def run_pipeline(engine: str, windows: List[np.ndarray], n_groups, k: int, horizon: int = 3, group_cap: int = 8):
    """The windows through ``WindowPipeline(engine, exemplars=k)`` and a ``RingWindowSource`` over a
    span ring. ``n_groups``: one number, or one per window. Returns (per-window results, per-window
    tracker results; the latter empty with ``k`` = 0)."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import Cut, RingWindowSource, WindowPipeline
    from llm_slo_ebpf_toolkit_amd.runtime import load

    rt = load()
    pipe = WindowPipeline(4096, 1024, group_cap, model="bayes", learn=False, user_cap=1024, engine=engine,
                          ttft_slo_ms=800.0, window_ms=1000.0, exemplars=k, exemplar_windows=horizon)
    ring = rt.HostRing(1 << 12, 64)
    src = RingWindowSource(pipe, None, None, ring)
    res, exs = [], []
    try:
        for w, recs in enumerate(windows):
            G = n_groups if np.isscalar(n_groups) else n_groups[w]
            assert ring.push(recs) == len(recs)
            kk = src.stage(Cut(kernel=0, user=0, spans=ring.head), G)["k"]
            res.append({key: np.array(v, copy=True) for key, v in pipe.results(kk, G).items()})
            if k:
                exs.append({key: np.array(v, copy=True) for key, v in pipe.exemplar_results(kk, G).items()})
        src.drain()
    finally:
        pipe.close()
    return res, exs
