#!/usr/bin/env python3
"""Device time of one open-request tracker step (ops/openreq.py), device events around ``step``.

The benchmark's span shape: 16,384 spans per window -- a third of them start records, a third
first-token records (counted), a third request spans (not counted) -- into a table of 2^20
entries that holds ~50,000 live rows in the steady state (requests whose first token comes about
nine windows after their start: most rows are past their deadline and counted, the worst case for
the resolve pass). Prints the median, min and max of the timed steps after the warm-up, copy +
kernels and kernels alone, as one JSON line.

    python tools/openreq_step_bench.py [--steps 200] [--warmup 30] [--spans 16384] [--cap 1048576] [--live 50000]
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--spans", type=int, default=16384)
    ap.add_argument("--cap", type=int, default=1 << 20)
    ap.add_argument("--live", type=int, default=50000)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args(argv)

    from llm_slo_ebpf_toolkit_amd.collector import records as R
    from llm_slo_ebpf_toolkit_amd.ops.openreq import OpenRequestTable
    from llm_slo_ebpf_toolkit_amd.pipeline.openreq import stats_dict

    rng = np.random.default_rng(a.seed)
    per = a.spans // 3                       # requests starting per window
    hold = max(1, round(a.live / per))       # windows a request stays open
    n_win = a.warmup + a.steps + hold
    T0, W = 1_700_000_000_000_000_000, 1_000_000_000
    th = rng.integers(1, 1 << 63, size=(n_win, per), dtype=np.uint64) | np.uint64(1)
    grp = rng.integers(0, a.groups, size=(n_win, per)).astype(np.uint32)
    start = T0 + np.arange(n_win)[:, None] * W + rng.integers(1, W, size=(n_win, per))
    ttft = np.float32(hold * 1e3)

    def window(w: int) -> np.ndarray:
        parts = []
        s = np.zeros(per, R.SPAN)
        s["ts_ns"], s["trace_h"], s["group_id"], s["ttft_ms"] = start[w], th[w], grp[w], np.nan
        s["flags"] = R.SPAN_START | R.SPAN_NO_SLI
        parts.append(s)
        if w >= hold:  # the requests of `hold` windows ago report: first token, then the request span
            for fl in (R.SPAN_FIRST_TOKEN | R.SPAN_LATE, R.SPAN_NO_SLI | R.SPAN_LATE):
                f = np.zeros(per, R.SPAN)
                f["ts_ns"], f["trace_h"], f["group_id"], f["ttft_ms"] = start[w - hold], th[w - hold], grp[w - hold], ttft
                f["flags"] = fl
                parts.append(f)
        out = np.concatenate(parts)
        return np.ascontiguousarray(out[rng.permutation(len(out))])

    t = OpenRequestTable(cap=a.cap, span_cap=a.spans, group_cap=a.groups, n_buffers=3, slo_ms=800.0)
    both, kern, live, n_sp = [], [], [], []
    prev = 0
    for w in range(a.warmup + a.steps):
        spans = window(w)
        cut = T0 + (w + 1) * W
        i = t.step_records(spans, cut, prev, a.groups)
        prev = cut
        r = t.results(i, a.groups)
        if w >= a.warmup:
            ms = t.step_ms(i)
            both.append(ms[0])
            kern.append(ms[1])
            st = stats_dict(r["stats"])
            live.append(st["live_open"] + st["live_counted"] + st["live_resolved"])
            n_sp.append(len(spans))
            assert st["dropped_full"] == 0 and st["marker_dropped"] == 0
    t.close()
    us = lambda v: round(1e3 * float(v), 2)  # noqa: E731
    print(json.dumps({"metric": "openreq_step_us", "steps": a.steps, "warmup": a.warmup, "cap": a.cap,
                      "spans_per_window": int(np.median(n_sp)), "live_entries": int(np.median(live)),
                      "step_us_median": us(np.median(both)), "step_us_min": us(np.min(both)),
                      "step_us_max": us(np.max(both)), "kernels_us_median": us(np.median(kern)),
                      "kernels_us_min": us(np.min(kern)), "kernels_us_max": us(np.max(kern))}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
