#!/usr/bin/env python3
"""Device time of one saturation curve step (ops/satcurve.py), device events around ``step``.

The benchmark's span shape: 16,383 spans per window over 64 services, half of them records that end a
request (observed: log-normal durations, median 800 ms with a heavy tail, a TTFT of three tenths of the
duration, ends spread over the window's 4 bins) and half first-token records (skipped), a ring of 1,024
bins of 500 ms, generations of ``--epoch-bins`` bins, cuts one window apart.
Prints the median, min and max of the timed steps after the warm-up -- copy + kernels, kernels alone
and the observe kernel alone -- as one JSON line. ``--shape one-bin`` times the contention shape instead
(every record observed, one service, every end in one bin), ``--shape four-bins`` one service with its
ends over the window's 4 bins, ``--shape long`` 64 services with 10 s requests; ``--no-lds`` runs the
observe kernel without its per-workgroup LDS table, the measurement's other side.

    python tools/satcurve_step_bench.py [--steps 200] [--warmup 30] [--spans 16383] [--groups 64] [--bins 1024]
        [--window-bins 4] [--epoch-bins 43200] [--shape bench|one-bin|four-bins|long] [--no-lds]
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
    ap.add_argument("--spans", type=int, default=16383)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--window-bins", type=int, default=4)
    ap.add_argument("--bin-ms", type=float, default=500.0)
    ap.add_argument("--epoch-bins", type=int, default=43200)
    ap.add_argument("--shape", choices=("bench", "one-bin", "four-bins", "long"), default="bench")
    ap.add_argument("--no-lds", action="store_true")
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args(argv)

    from llm_slo_ebpf_toolkit_amd.collector import records as R
    from llm_slo_ebpf_toolkit_amd.ops.satcurve import SaturationTracker
    from llm_slo_ebpf_toolkit_amd.pipeline.satcurve import stats_dict

    rng = np.random.default_rng(a.seed)
    bin_us = int(round(a.bin_ms * 1e3))
    q_start = 1_700_000_000_000_000 // bin_us

    def window():
        """(records, microseconds from the end of the cut's bin back to each record's end): the start times are
        set per step."""
        s = np.zeros(a.spans, R.SPAN)
        s["trace_h"] = rng.integers(1, 1 << 63, a.spans, dtype=np.uint64)
        s["ttft_ms"] = np.float32(300.0)  # the one-service shapes: inside the SLO
        back = rng.integers(1, a.window_bins * bin_us, a.spans)
        if a.shape == "bench":
            s["latency_ms"] = np.minimum(rng.lognormal(np.log(800.0), 1.0, a.spans), 60_000.0).astype(np.float32)
            s["ttft_ms"] = s["latency_ms"] * np.float32(0.3)
            s["group_id"] = rng.integers(0, a.groups, a.spans)
            s["flags"] = np.where(np.arange(a.spans) % 2 == 0, R.SPAN_NO_SLI, R.SPAN_FIRST_TOKEN)
            p = rng.permutation(a.spans)
            return np.ascontiguousarray(s[p]), back[p]
        if a.shape == "long":
            s["latency_ms"] = np.float32(10_000.0)
            s["group_id"] = rng.integers(0, a.groups, a.spans)
            return s, back
        s["latency_ms"] = np.float32(100.0)
        return s, (rng.integers(1, bin_us, a.spans) if a.shape == "one-bin" else back)

    pool = [window() for _ in range(8)]
    t = SaturationTracker(bins=a.bins, bin_us=bin_us, epoch_bins=a.epoch_bins, span_cap=max(a.spans, 1), group_cap=a.groups,
                          n_buffers=3, lds=not a.no_lds)
    both, kern, obs, seen = [], [], [], []
    for w in range(a.warmup + a.steps):
        q_hi = q_start + a.window_bins * (w + 1)
        recs, back = pool[w % len(pool)]
        end_us = (q_hi + 1) * bin_us - back
        dur_us = np.trunc(recs["latency_ms"].astype(np.float64) * 1000.0).astype(np.int64)
        recs["ts_ns"] = (end_us - dur_us) * 1000
        i = t.step_records(recs, (q_hi * bin_us + bin_us - 1) * 1000, a.groups)
        r = t.results(i, a.groups)
        if w >= a.warmup:
            ms = t.step_ms(i)
            both.append(ms[0])
            kern.append(ms[1])
            obs.append(t.observe_ms(i))
            seen.append(stats_dict(r["stats"])["observed"])
    rows = r["rows"]
    t.close()
    us = lambda v: round(1e3 * float(v), 2)  # noqa: E731
    out = {"metric": "satcurve_step_us", "shape": a.shape, "lds": not a.no_lds, "steps": a.steps, "warmup": a.warmup,
           "groups": a.groups, "bins": a.bins, "window_bins": a.window_bins, "bin_ms": a.bin_ms,
           "spans_per_window": a.spans, "observed_per_window": int(np.median(seen)),
           "epoch_bins": a.epoch_bins, "curve_requests": int(rows["n_total"].sum()), "curve_breaches": int(rows["b_total"].sum()),
           "knees": int((rows["knee_level"] != 0xFFFFFFFF).sum()), "states": np.bincount(rows["state"], minlength=4).tolist(),
           "last_stats": stats_dict(r["stats"])}
    for name, v in (("step", both), ("kernels", kern), ("observe", obs)):
        out.update({f"{name}_us_median": us(np.median(v)), f"{name}_us_min": us(np.min(v)),
                    f"{name}_us_max": us(np.max(v))})
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
