"""Per-service TTFT distributions (pipeline/slisketch.py): the rules on the host implementation
against brute force -- histograms, ``le`` counts, sums, quantiles within the derived 1/32, the edge
values, eviction -- then the window pipeline's new keys and unchanged defaults, the agent's flags,
series and decision-log field, and the sketch's host side under the host sanitizers.
tests/test_slisketch_gpu.py holds the device sketch against this implementation."""

import os

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.pipeline import slisketch as sk
from llm_slo_ebpf_toolkit_amd.pipeline.oracle import milli_units
from tests import slisketch_scenarios as sc

REL = 1.0 / 32.0  # a value in buckets 1..384 against its bucket's midpoint (docs/TTFT_DISTRIBUTION.md)


def _check_against_brute_force(res, grp, v, G, what):
    """``res`` = (hist [C, K], quantile buckets [G, 4]) against the records (grp, v) themselves."""
    hist, q = res
    np.testing.assert_array_equal(hist, sc.brute_hist(grp, v, hist.shape[0]), err_msg=what)
    q_ms = sk.representative()
    for g in range(G):
        x = v[grp == g]
        if not len(x):
            assert (q[g] == sk.EMPTY).all(), what
            continue
        for j, exact in enumerate(sc.exact_quantiles(x)):
            got = q_ms[int(q[g, j])]
            assert int(q[g, j]) == int(sk.bucket_of(np.float32(exact))), what
            if 0.125 <= exact < 2.0 ** 21:
                assert abs(got - exact) <= REL * exact, (what, g, j, got, exact)


def test_oracle_equals_brute_force_every_window_and_over_the_horizon():
    rng = np.random.default_rng(11)
    G, C, W = 4, 6, 3
    o = sk.SliSketchOracle(span_cap=4096, group_cap=C, windows=W)
    wins = [sc.window(rng, int(n), G, C) for n in (200, 5, 0, 900, 64, 1, 333)]
    obs = []
    for w, recs in enumerate(wins):
        r = o.results(o.step_records(recs, G), G)
        grp, v, n_counted, n_invalid, n_out = sc.counted(recs, G)
        obs.append((grp, v))
        _check_against_brute_force((o.window_hist().astype(np.int64), r["q_win"]), grp, v, G, f"window {w}")
        hg = np.concatenate([a for a, _ in obs[-W:]])
        hv = np.concatenate([b for _, b in obs[-W:]])
        _check_against_brute_force((o.rolling().astype(np.int64), r["q_roll"]), hg, hv, G, f"horizon at {w}")
        np.testing.assert_array_equal(r["n"], np.bincount(grp, minlength=G)[:G])
        np.testing.assert_array_equal(r["n_roll"], np.bincount(hg, minlength=G)[:G])
        edges = np.array(sk.EDGES, np.float32)
        for g in range(G):
            x = v[grp == g]
            cum = [(x <= e).sum() for e in edges] + [len(x)]
            np.testing.assert_array_equal(np.cumsum(r["le"][g]), cum, err_msg=f"window {w} group {g} le")
            assert int(r["sum_milli"][g]) == int(milli_units(np.minimum(x, np.float32(2 ** 21))).sum())
        st = sk.stats_dict(r["stats"])
        assert st["observed"] == len(v) == n_counted - n_invalid and st["invalid"] == n_invalid
        assert st["out_of_group"] == n_out == 2
        assert st["underflow"] == int((sk.bucket_of(v) == 0).sum())
        assert st["overflow"] == int((sk.bucket_of(v) == sk.K - 1).sum())


def test_the_relative_error_bound_on_log_normal_sets():
    """The midpoint of a bucket of width lo / 16 is at most lo / 32 from any value >= lo in it."""
    rng = np.random.default_rng(5)
    rep = sk.representative()
    worst = 0.0
    for _ in range(50):
        v = rng.lognormal(rng.uniform(0, 9), rng.uniform(0.2, 2.5), 400).astype(np.float32)
        v = v[(v >= 0.125) & (v < 2.0 ** 21)]
        worst = max(worst, float(np.max(np.abs(rep[sk.bucket_of(v)] - v.astype(np.float64)) / v.astype(np.float64))))
    assert worst <= REL
    e = sk.bucket_edges()
    assert e[0] == 0.125 and e[-1] == 2.0 ** 21 and len(e) == sk.NB + 1 and (np.diff(e) > 0).all()
    assert ((e[1:] - e[:-1]) / e[:-1] <= 1.0 / 16.0).all()


def test_edge_values_land_where_the_rule_says():
    f = np.float32
    for v, where in sc.EDGE_VALUES:
        if where == "invalid":
            continue
        b = int(sk.bucket_of(v))
        assert {"under": b == 0, "over": b == sk.K - 1, "in": 1 <= b <= sk.NB}[where], (v, b)
    assert int(sk.bucket_of(f(0.125))) == 1 and int(sk.bucket_of(np.nextafter(f(2 ** 21), f(0)))) == sk.NB
    # 800 = 1.5625 x 2^9 is a bucket's lower edge
    b800 = int(sk.bucket_of(f(800.0)))
    assert int(sk.bucket_of(np.nextafter(f(800), f(0)))) == b800 - 1 and sk.bucket_edges()[b800 - 1] == 800.0
    assert int(sk.bucket_of(np.nextafter(f(800), f(np.inf)))) == b800
    o = sk.SliSketchOracle(span_cap=64, group_cap=2, windows=2)
    vals = [v for v, _ in sc.EDGE_VALUES]
    recs = np.concatenate([sc.spans(vals, [0] * len(vals)),
                           sc.spans([100.0, 100.0], [0, 0], R.SPAN_NO_SLI),
                           sc.spans([np.nan], [0], R.SPAN_START | R.SPAN_NO_SLI),
                           sc.spans([100.0, 100.0, 100.0], [1, 2, 9]),
                           sc.spans([5000.0], [0], R.SPAN_FIRST_TOKEN | R.SPAN_LATE)])
    r = o.results(o.step_records(recs, 1), 1)
    st = sk.stats_dict(r["stats"])
    n_valid = sum(w != "invalid" for _, w in sc.EDGE_VALUES)
    assert st == {"observed": n_valid + 1, "invalid": 2, "underflow": 4, "overflow": 3, "out_of_group": 3}
    assert int(r["n"][0]) == n_valid + 1  # the SPAN_LATE record counts by its value
    h = o.window_hist()[0]
    assert h[0] == 4 and h[sk.K - 1] == 3 and h[1] == 2 and h[sk.NB] == 1 and h[b800] == 2 and h[b800 - 1] == 1
    assert not o.window_hist()[1].any()
    # le: 0, -0, denormal, < 0.125, 0.125, > 0.125 | 800-, 800 | 800+ | 5000, 2^21-, 2^21, 2^21+, inf
    assert r["le"][0].tolist() == [6, 0, 0, 0, 2, 1, 0, 5]
    # +inf and 2^21+ enter the sum clamped to 2^21
    want = sum(int(milli_units(np.minimum(np.float32(v), np.float32(2 ** 21)))) for v in vals
               if v >= 0) + 5_000_000
    assert int(r["sum_milli"][0]) == want
    qw, qr = sk.quantiles_ms(r)
    assert qw.shape == (1, 4) and np.array_equal(qw, qr) and qw[0, 3] == 2.0 ** 21


def test_horizon_of_one_window_is_the_window():
    rng = np.random.default_rng(2)
    o = sk.SliSketchOracle(span_cap=1024, group_cap=3, windows=1)
    for n in (50, 0, 7):
        r = o.results(o.step_records(sc.window(rng, n, 3, 3, edges=False), 3), 3)
        np.testing.assert_array_equal(o.rolling(), o.window_hist())
        np.testing.assert_array_equal(r["q_win"], r["q_roll"])
        np.testing.assert_array_equal(r["n"], r["n_roll"])


def test_eviction_with_an_empty_step_and_changing_groups():
    """W = 3 over 8 steps: every step evicts the step 3 before it in every row, also when the step
    is empty or the row's group is absent from it."""
    rng = np.random.default_rng(3)
    C, W = 5, 3
    groups = [5, 5, 0, 5, 2, 5, 5, 2]
    sizes = [40, 30, 25, 0, 35, 20, 0, 10]
    o = sk.SliSketchOracle(span_cap=1024, group_cap=C, windows=W)
    hists = []
    for w, (G, n) in enumerate(zip(groups, sizes)):
        recs = sc.window(rng, n, G, C, edges=w % 2 == 0)
        r = o.results(o.step_records(recs, G), G)
        grp, v, *_ = sc.counted(recs, G)
        hists.append(sc.brute_hist(grp, v, C))
        want = np.sum(hists[-W:], axis=0)
        np.testing.assert_array_equal(o.rolling(), want, err_msg=f"step {w}")
        np.testing.assert_array_equal(o.window_hist(), hists[-1], err_msg=f"step {w}")
        np.testing.assert_array_equal(r["n_roll"], want.sum(axis=1)[:G])
        np.testing.assert_array_equal(r["q_roll"], sk.rank_buckets(want)[:G])
    assert not hists[2].any() and not hists[3].any()  # n_groups = 0, and the empty step
    assert hists[4][2:].sum() == 0 and o.rolling()[2:].sum() == hists[5][2:].sum() + hists[6][2:].sum()


def test_oracle_checks_its_arguments_and_keeps_the_last_steps():
    for kw in (dict(windows=0), dict(windows=4097), dict(group_cap=0), dict(group_cap=65537), dict(n_buffers=0),
               dict(span_cap=0), dict(span_cap=1 << 20, windows=4096, group_cap=1),
               dict(windows=4096, group_cap=512, span_cap=16)):
        with pytest.raises(ValueError):
            sk.SliSketchOracle(**kw)
    o = sk.SliSketchOracle(span_cap=4, group_cap=2, windows=2, n_buffers=2)
    none = np.zeros(0, R.SPAN)
    with pytest.raises(ValueError):
        o.step_records(none, 3)
    with pytest.raises(ValueError):
        o.step_records(np.zeros(5, R.SPAN), 2)
    with pytest.raises(ValueError):
        o.step([(1 << 20, 63)], 2)
    assert o.n == 0  # a refused step is no step
    for i in range(3):
        assert o.step_records(sc.spans([100.0 * (i + 1)], [1]), 2) == i
    assert set(o.results(2, 2)) == set(sk.RESULT_FIELDS)
    assert o.results(2, 2)["n"].tolist() == [0, 1] and o.results(1, 1)["le"].shape == (1, 8)
    assert o.results(2, 2)["n_roll"].tolist() == [0, 2]
    with pytest.raises(IndexError):
        o.results(0, 2)
    with pytest.raises(IndexError):
        o.results(3, 2)


# ---- the window pipeline ---------------------------------------------------------------------------

RESULT_KEYS = {"post", "conf", "feat", "pred", "evbits", "sli", "app", "late"}


def _stream(seed=7, n_windows=6, G=3):
    rng = np.random.default_rng(seed)
    return [sc.window(rng, int(n), G, 8, edges=False) for n in rng.integers(0, 60, n_windows)]


def test_pipeline_on_the_host_engine_carries_the_new_keys_only_when_switched_on():
    from llm_slo_ebpf_toolkit_amd.pipeline.window import WindowPipeline

    G, W = 3, 2
    wins = _stream()
    off, none = sc.run_pipeline("cpu", wins, G, 0)
    on, sks = sc.run_pipeline("cpu", wins, G, W)
    both, _ = sc.run_pipeline("cpu", wins, G, W, open_requests=1 << 10)
    ref = sk.SliSketchOracle(span_cap=1024, group_cap=8, windows=W)
    assert none == []
    for w, (a, b, c, s) in enumerate(zip(off, on, both, sks)):
        assert set(a) == RESULT_KEYS, "sketch off: today's keys"
        assert set(b) == RESULT_KEYS | set(sk.RESULT_KEYS)
        assert set(c) == set(b) | {"sli_raw", "late_raw", "deadline", "deadline_dup"}
        for key in RESULT_KEYS:
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"window {w} {key}")
        want = ref.results(ref.step_records(wins[w], G), G)
        for key in sk.RESULT_FIELDS:
            np.testing.assert_array_equal(s[key], want[key], err_msg=f"window {w} {key}")
        for key, val in sk.result_keys(want).items():
            np.testing.assert_array_equal(b[key], val, err_msg=f"window {w} {key}")
            np.testing.assert_array_equal(c[key], val, err_msg=f"window {w} {key}")
        # no invalid record on this stream: the sketch holds every request the engine counted
        np.testing.assert_array_equal(b["ttft_n"], b["sli"][:, 0] + b["late"][:, 0], err_msg=f"window {w}")
        np.testing.assert_array_equal(c["ttft_n"], c["sli_raw"][:, 0] + c["late_raw"][:, 0], err_msg=f"window {w}")
        assert b["ttft_q"].shape == (G, 4) and b["ttft_le"].shape == (G, 8) and b["ttft_sum_ms"].dtype == np.float64
        assert np.isnan(b["ttft_q"][b["ttft_n"] == 0]).all() and np.isfinite(b["ttft_q"][b["ttft_n"] > 0]).all()
    assert sum(int(r["ttft_n"].sum()) for r in on) > 50
    # one GPU only: a communicator or a shard of a node's stream is refused
    with pytest.raises(ValueError, match="one GPU"):
        WindowPipeline(1024, 64, 4, engine="cpu", shard=(0, 2), sli_sketch=5)


# ---- the agent ----------------------------------------------------------------------------------------

def test_agent_flags_and_the_one_gpu_rule():
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions
    from llm_slo_ebpf_toolkit_amd.cli.agent import parse

    o, _ = parse(["--engine", "cpu", "--ttft-distribution", "--ttft-horizon-windows", "40"])
    assert o.ttft_distribution and o.ttft_horizon_windows == 40
    d = parse([])[0]
    assert not d.ttft_distribution and d.ttft_horizon_windows == 0 and not AgentOptions().ttft_distribution
    def mk(**kw):
        return Agent(AgentOptions(engine="cpu", source="replay", config="", output="stdout", metrics_bind="",
                                  ring_name=f"/mislo-sk2-{os.getpid()}", **kw))

    a = mk(gpus=1, window_ms=2000)
    try:
        assert a.ttft_horizon() == 150  # 5 minutes of 2 s windows
        a.o.window_ms, a.o.ttft_horizon_windows = 300, 0
        assert a.ttft_horizon() == 1000
        a.o.ttft_horizon_windows = 12
        assert a.ttft_horizon() == 12
    finally:
        a.close()
    a = mk(gpus=2, ttft_distribution=True)
    try:
        with pytest.raises(ValueError, match="one GPU"):
            a.run_windows(max_windows=1)
    finally:
        a.close()


@pytest.mark.timeout(120)
def test_agent_runs_with_ttft_distribution_and_exports_the_series(tmp_path):
    import io
    import json

    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions
    from llm_slo_ebpf_toolkit_amd.export.prometheus import parse_exposition

    log = tmp_path / "decisions.jsonl"
    o = AgentOptions(engine="cpu", source="replay", gpus=1, window_events=2048, window_spans=128, window_groups=8,
                     window_ms=300, metrics_bind="", output="stdout", ring_name=f"/mislo-sk1-{os.getpid()}",
                     config="", min_confidence=0.0, scenario="full", disable_overhead_guard=True,
                     ttft_distribution=True, ttft_horizon_windows=3, decision_log=str(log))
    a = Agent(o, out_stream=io.StringIO())
    try:
        assert a.run_windows(max_windows=4) == 0
    finally:
        a.close()
    res = a.last_results
    assert set(sk.RESULT_KEYS) <= set(res) and "deadline" not in res
    np.testing.assert_array_equal(res["ttft_n"], res["sli"][:, 0] + res["late"][:, 0])
    m = parse_exposition(a.metrics.registry.exposition())
    count = {k: v for k, v in m.items() if k.startswith("llm_slo_agent_ttft_ms_count{")}
    assert count and sum(count.values()) > 0
    svc = next(k for k, v in count.items() if v > 0).split("{", 1)[1].rstrip("}")
    assert m[f'llm_slo_agent_ttft_ms_bucket{{{svc},le="+Inf"}}'] == count[f"llm_slo_agent_ttft_ms_count{{{svc}}}"]
    assert m[f'llm_slo_agent_ttft_ms_bucket{{{svc},le="800"}}'] <= m[f'llm_slo_agent_ttft_ms_bucket{{{svc},le="+Inf"}}']
    assert m[f"llm_slo_agent_ttft_ms_sum{{{svc}}}"] > 0
    for scope in ("window", "rolling"):
        p50 = m[f'llm_slo_agent_ttft_quantile_ms{{{svc},quantile="0.5",scope="{scope}"}}']
        p99 = m[f'llm_slo_agent_ttft_quantile_ms{{{svc},quantile="0.99",scope="{scope}"}}']
        assert 0 < p50 <= p99
    for reason in sk.EVENT_STATS:
        assert m[f'llm_slo_agent_ttft_sketch_events_total{{reason="{reason}"}}'] == 0
    rows = [json.loads(ln) for ln in log.read_text().splitlines()]
    assert rows and all(set(r["ttft_ms"]) == {"n", "p50", "p95", "p99", "p95_5m"} for r in rows)
    busy = [r for r in rows if r["ttft_ms"]["n"] > 0]
    assert busy and all(r["ttft_ms"]["p50"] <= r["ttft_ms"]["p95"] <= r["ttft_ms"]["p99"] for r in busy)
    assert all(r["ttft_ms"]["p95_5m"] is not None for r in busy)


def test_ttft_metrics():
    from llm_slo_ebpf_toolkit_amd.agent.metrics import AgentMetrics
    from llm_slo_ebpf_toolkit_amd.evaluation.slo import histogram_quantile
    from llm_slo_ebpf_toolkit_amd.export.prometheus import parse_exposition

    o = sk.SliSketchOracle(span_cap=64, group_cap=2, windows=4)
    m = AgentMetrics("probe", "auto", [], [])
    for vals in ([40.0, 90.0, 700.0, 900.0, 2500.0], [60.0, float("nan")]):
        r = o.results(o.step_records(sc.spans(vals, [0] * len(vals)), 2), 2)
        m.observe_ttft(sk.result_keys(r), sk.stats_dict(r["stats"]), ["rag"])
    v = parse_exposition(m.registry.exposition())
    cum = [v[f'llm_slo_agent_ttft_ms_bucket{{service="rag",le="{e}"}}'] for e in
           ("50", "100", "200", "400", "800", "1200", "2000", "+Inf")]
    assert cum == [1, 3, 3, 3, 4, 5, 5, 6] and v['llm_slo_agent_ttft_ms_count{service="rag"}'] == 6
    assert v['llm_slo_agent_ttft_ms_sum{service="rag"}'] == pytest.approx(4290.0)
    assert histogram_quantile(0.5, list(sk.EDGES) + [float("inf")], cum) == pytest.approx(100.0)
    q = 'llm_slo_agent_ttft_quantile_ms{service="rag",quantile="%s",scope="%s"}'
    assert v[q % ("0.5", "window")] == pytest.approx(60.0, rel=REL)
    assert v[q % ("0.5", "rolling")] == pytest.approx(90.0, rel=REL)
    assert v[q % ("0.99", "rolling")] == pytest.approx(2500.0, rel=REL)
    assert not any(k.startswith('llm_slo_agent_ttft_quantile_ms{service="group-1"') for k in v)  # never a NaN
    assert v['llm_slo_agent_ttft_sketch_events_total{reason="invalid"}'] == 1
    assert v['llm_slo_agent_ttft_sketch_events_total{reason="overflow"}'] == 0


# ---- the sketch's host side under the host sanitizers ---------------------------------------------

@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="needs g++")
@pytest.mark.timeout(300)
def test_sketch_host_side_under_address_and_ub_sanitizers(tmp_path):
    """ops/csrc/slisketch_host.h (bucket rule, argument checks, result layout) needs no device: a
    stand-alone program over it, built with AddressSanitizer + UBSan."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "llm_slo_ebpf_toolkit_amd", "ops", "csrc")
    exe = tmp_path / "slisketch_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-Wall", "-Werror", f"-I{csrc}", os.path.join(root, "tests", "native", "slisketch_host_check.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "slisketch host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
