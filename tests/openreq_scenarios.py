"""Request streams for the open-request tracker's tests (pipeline/openreq.py, ops/openreq.py): a
seeded service that exports, per request, a start record at the request's start, a first-token
record (the counted one) when the first token is out and the request span (SPAN_NO_SLI) a little
later -- each placed in the window it arrives in, flagged SPAN_LATE by the receiver's rule
(collector/otlp.py: the deadline lies before the agent's last cut)."""

from dataclasses import dataclass, field
from typing import List

import numpy as np

from llm_slo_ebpf_toolkit_amd.collector import records as R

T0 = 1_700_000_000_000_000_000
WINDOW_NS = 1_000_000_000
SLO_MS = 800.0
MS = 1_000_000


@dataclass
class Stream:
    windows: List[np.ndarray]     # SPAN records per window, in arrival order
    cuts: List[int]               # cut time of each window
    n_groups: int
    n_requests: int
    n_breaching: int
    fault_window: int
    fault_group: int
    trace_h: np.ndarray = field(default=None)
    start: np.ndarray = field(default=None)
    ttft_ms: np.ndarray = field(default=None)
    grp: np.ndarray = field(default=None)


def cut_of(w: int) -> int:
    return T0 + (w + 1) * WINDOW_NS


def span(ts, trace_h, grp, ttft_ms, flags) -> np.ndarray:
    r = np.zeros(1, dtype=R.SPAN)
    r["ts_ns"], r["trace_h"], r["group_id"], r["ttft_ms"], r["flags"] = ts, trace_h, grp, ttft_ms, flags
    r["pod_id"], r["pid"], r["svc_id"] = 7 + int(grp), 4000 + int(grp), int(grp) + 1
    r["span_h"] = (int(trace_h) * 3 + int(flags)) & ((1 << 64) - 1)
    r["latency_ms"] = 0.0 if flags & R.SPAN_START else ttft_ms
    return r


def stream(seed=5, n_groups=3, per_window=30, n_windows=12, fault_window=5, fault_group=1, late_ms=3500.0,
           healthy_ms=100.0, send_windows=None, starts=True, tail_ms=50.0, flag_late=True) -> Stream:
    """``per_window`` requests start in each of the first ``send_windows`` windows (default: all but
    the last 5, so every request reports before the stream ends); from ``fault_window`` on the
    first tokens of ``fault_group`` come ``late_ms`` after the start, the rest ``healthy_ms``.
    ``flag_late=False``: a service that pushes its records into the span ring itself, past the
    receiver -- no record carries SPAN_LATE."""
    rng = np.random.default_rng(seed)
    send = n_windows - 5 if send_windows is None else send_windows
    n = per_window * send
    w_of = np.repeat(np.arange(send), per_window)
    start = T0 + w_of * WINDOW_NS + np.sort(rng.integers(1, WINDOW_NS, size=(send, per_window)), axis=1).ravel()
    grp = rng.integers(0, n_groups, size=n)
    th = rng.integers(1, 1 << 63, size=n, dtype=np.uint64) | np.uint64(1)
    assert len(np.unique(th)) == n
    slow = (grp == fault_group) & (w_of >= fault_window)
    ttft = np.where(slow, late_ms, healthy_ms)
    # arrivals: (time, order within a request, record)
    arr = []
    slo_ns = int(SLO_MS * MS)
    for i in range(n):
        t, h, g, v = int(start[i]), int(th[i]), int(grp[i]), float(ttft[i])
        if starts:
            arr.append((t, 0, span(t, h, g, np.nan, R.SPAN_START | R.SPAN_NO_SLI)))
        for k, (at, fl) in enumerate(((t + int(v * MS), R.SPAN_FIRST_TOKEN),
                                      (t + int((v + tail_ms) * MS), R.SPAN_NO_SLI)), start=1):
            last_cut = T0 + ((at - T0) // WINDOW_NS) * WINDOW_NS  # the agent's last cut when it arrives
            if flag_late and last_cut > T0 and t + slo_ns < last_cut:
                fl |= R.SPAN_LATE
            arr.append((at, k, span(t, h, g, v, fl)))
    arr.sort(key=lambda x: (x[0], x[1]))
    wins = [[] for _ in range(n_windows)]
    for at, _k, rec in arr:
        w = (at - T0) // WINDOW_NS
        assert w < n_windows, "the stream ends before every request reported"
        wins[w].append(rec)
    windows = [np.concatenate(w) if w else np.zeros(0, R.SPAN) for w in wins]
    return Stream(windows=windows, cuts=[cut_of(w) for w in range(n_windows)], n_groups=n_groups, n_requests=n,
                  n_breaching=int((ttft > SLO_MS).sum()), fault_window=fault_window, fault_group=fault_group,
                  trace_h=th, start=start, ttft_ms=ttft, grp=grp)


def engine_counts(spans: np.ndarray, n_groups: int, slo_ms: float = SLO_MS):
    """sli [G, 2] and late [G, 2] as both window engines count a window's spans (k_decode_spans,
    pipeline/cpu.py)."""
    sli, late = np.zeros((n_groups, 2), np.uint32), np.zeros((n_groups, 2), np.uint32)
    g = spans["group_id"].astype(np.int64)
    ok = ((spans["flags"] & np.uint32(R.SPAN_NO_SLI)) == 0) & (g < n_groups)
    breach = spans["ttft_ms"] > np.float32(slo_ms)
    is_late = breach & ((spans["flags"] & np.uint32(R.SPAN_LATE)) != 0)
    np.add.at(sli[:, 0], g[ok & ~is_late], 1)
    np.add.at(sli[:, 1], g[ok & breach & ~is_late], 1)
    np.add.at(late[:, 0], g[ok & is_late], 1)
    return sli, late


def run(tracker, st: Stream, each=None):
    """Every window of ``st`` through ``tracker``; ``each(w, results)`` after each step. Returns the
    per-window tracker results."""
    out = []
    prev = 0
    for w, (spans, cut) in enumerate(zip(st.windows, st.cuts)):
        i = tracker.step_records(spans, cut, prev, st.n_groups)
        prev = cut
        res = tracker.results(i, st.n_groups)
        out.append(res)
        if each is not None:
            each(w, res)
    return out


def run_pipeline(engine: str, st: Stream, tag: str, cap: int = 1 << 12):
    """The stream through ``WindowPipeline(engine, open_requests=cap)`` and a ``RingWindowSource``
    over a span ring, the cuts carrying their times; one more cut without a time at the end (a
    replay helper's: skipped). Returns (per-window results, per-window tracker stats, counters)."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import Cut, RingWindowSource, WindowPipeline
    from llm_slo_ebpf_toolkit_amd.runtime import load

    rt = load()
    pipe = WindowPipeline(4096, 1024, 8, model="bayes", learn=False, user_cap=1024, engine=engine,
                          ttft_slo_ms=SLO_MS, window_ms=1000.0, open_requests=cap)
    spans = rt.HostRing(1 << 12, 64)
    src = RingWindowSource(pipe, None, None, spans)
    res, stats = [], []
    for w, (recs, cut) in enumerate(zip(st.windows, st.cuts)):
        assert spans.push(recs) == len(recs)
        k = src.stage(Cut(kernel=0, user=0, spans=spans.head, t_ns=cut), st.n_groups)["k"]
        res.append({key: np.array(v, copy=True) for key, v in pipe.results(k, st.n_groups).items()})
        stats.append(np.array(pipe.open_results(k, st.n_groups)["stats"], copy=True))
    k = src.stage(Cut(kernel=0, user=0, spans=spans.head), st.n_groups)["k"]
    last = pipe.results(k, st.n_groups)
    assert not last["deadline"].any() and not last["deadline_dup"].any()
    src.drain()
    counters = {"skipped": pipe.open_skipped}
    pipe.close()
    return res, stats, counters
