"""Worst-TTFT request exemplars (pipeline/exemplars.py): the rules on the host implementation against
a brute-force lexsort -- window and recent rows, the edge values, ties, the horizon's wrap -- then
every refused configuration and step, the window pipeline's new keys and unchanged defaults, the
agent's incidents, decision log and series, the span mapper's trace-id memory, and the tracker's host
side under the host sanitizers. tests/test_exemplars_gpu.py holds the device tracker against this
implementation."""

import io
import json
import os

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.pipeline import exemplars as ex
from tests import exemplar_scenarios as sc

F32 = np.float32


def _ttfts(rows):
    return rows["ttft_ms"].tolist()


# ---- the oracle against brute force ------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("H", [1, 2, 3])
def test_oracle_equals_a_brute_force_lexsort_for_window_and_recent_rows(K, H):
    rng = np.random.default_rng(100 * K + H)
    G, C = 3, 5
    o = ex.ExemplarOracle(k=K, windows=H, span_cap=4096, group_cap=C)
    history = []
    for w, n in enumerate((60, 5, 0, 200, 2, 33, 90)):
        recs = sc.edge_window(rng, n, G) if w % 2 == 0 else sc.identify(sc.window(rng, n, G, C), rng)
        r = o.results(o.step_records(recs, G), G)
        n_want, rows = sc.brute_window(recs, G, C, K)
        np.testing.assert_array_equal(r["n"], n_want[:G], err_msg=f"window {w}")
        np.testing.assert_array_equal(r["k_win"], np.minimum(n_want, K)[:G], err_msg=f"window {w}")
        sc.same_rows(r["win"], rows[:G], f"window {w}")
        history.append((rows, np.minimum(n_want, K)))
        k_recent, recent = sc.brute_recent(history, C, K, H)
        np.testing.assert_array_equal(r["k_recent"], k_recent[:G], err_msg=f"horizon at {w}")
        sc.same_rows(r["recent"], recent[:G], f"horizon at {w}")
        st = ex.stats_dict(r["stats"])
        assert st["observed"] == len(sc.counted(recs, G)) == int(n_want.sum())
        if H == 1:
            sc.same_rows(r["recent"], r["win"], "a horizon of one window is the window")


def test_edge_values_rank_and_count_where_the_rule_says():
    vals = [F32(5.0), F32(-0.0), F32(np.inf), F32(0.0), F32(np.nan), F32(-1.0), F32(1e-40), F32(np.inf)]
    recs = np.concatenate([sc.spans(vals, [0] * len(vals)),
                           sc.spans([9000.0, 9000.0], [0, 0], R.SPAN_NO_SLI),               # counted elsewhere
                           sc.spans([np.nan], [0], R.SPAN_START | R.SPAN_NO_SLI),           # a start record
                           sc.spans([100.0, 100.0, 100.0], [1, 2, 9]),                      # group 1 of 2; out of group
                           sc.spans([7000.0], [0], R.SPAN_FIRST_TOKEN | R.SPAN_LATE)])      # late: by its value
    o = ex.ExemplarOracle(k=8, windows=2, span_cap=64, group_cap=4)
    r = o.results(o.step_records(recs, 2), 2)
    assert ex.stats_dict(r["stats"]) == {"observed": 8, "invalid": 2, "out_of_group": 2}
    assert r["n"].tolist() == [7, 1] and r["k_win"].tolist() == [7, 1]
    # +inf first (the earlier of the two), the late record by its value, -0.0 with 0.0 by index, last
    assert r["win"][0]["index"].tolist() == [2, 7, 14, 0, 6, 1, 3, 0]
    assert _ttfts(r["win"][0][:3]) == [np.inf, np.inf, 7000.0] and r["win"][0]["flags"][2] & R.SPAN_LATE
    assert np.signbit(r["win"][0]["ttft_ms"][5]) and not np.signbit(r["win"][0]["ttft_ms"][6])
    # fewer than K records: zero rows past the count
    assert not np.ascontiguousarray(r["win"][0][7:]).view(np.uint8).any()
    assert not np.ascontiguousarray(r["win"][1][1:]).view(np.uint8).any() and r["win"][1]["index"][0] == 11
    row = r["win"][0][3]
    src = recs[0]
    assert (row["trace_h"], row["span_h"], row["ts_ns"]) == (src["trace_h"], src["span_h"], src["ts_ns"])
    assert row["age"] == 0 and not row["pad"].any()
    keys = ex.window_keys([-0.0, 0.0, np.inf, 0.0], [3, 3, 9, (1 << 31) - 1]).tolist()
    assert keys[0] == keys[1] < keys[2] and keys[3] != 0 and keys[3] == 1 << 31


def test_equal_ttfts_go_to_the_earlier_record_and_across_windows_to_the_newer_window():
    o = ex.ExemplarOracle(k=3, windows=3, span_cap=64, group_cap=1)
    a = sc.spans([437.5] * 6, [0] * 6)
    a["span_h"] = np.arange(10, 16)
    r = o.results(o.step_records(a, 1), 1)
    assert r["win"][0]["index"].tolist() == [0, 1, 2] and r["recent"][0]["age"].tolist() == [0, 0, 0]
    b = sc.spans([437.5, 500.0, 437.5], [0] * 3)
    b["span_h"] = np.arange(20, 23)
    r = o.results(o.step_records(b, 1), 1)
    assert r["win"][0]["span_h"].tolist() == [21, 20, 22]
    # 500 first; of the 437.5s the newer window's, in its list's order, before the older window's
    assert r["recent"][0]["span_h"].tolist() == [21, 20, 22] and r["recent"][0]["age"].tolist() == [0, 0, 0]
    r = o.results(o.step_records(sc.spans([437.5], [0]), 1), 1)
    assert r["recent"][0]["age"].tolist() == [1, 0, 1] and r["recent"][0]["span_h"].tolist() == [21, 0, 20]
    r = o.results(o.step_records(np.zeros(0, R.SPAN), 1), 1)
    assert r["recent"][0]["age"].tolist() == [2, 1, 2] and r["k_win"][0] == 0 and r["n"][0] == 0
    r = o.results(o.step_records(np.zeros(0, R.SPAN), 1), 1)  # the window with 500 left the horizon
    assert r["k_recent"][0] == 1 and r["recent"][0]["age"].tolist() == [2, 0, 0]


def test_horizon_wraps_with_an_empty_step_and_a_step_without_groups_and_groups_age_out():
    rng = np.random.default_rng(9)
    C, K, H = 6, 3, 3
    groups = [6, 6, 0, 6, 2, 2, 2, 6]
    sizes = [40, 0, 30, 25, 20, 0, 20, 10]
    o = ex.ExemplarOracle(k=K, windows=H, span_cap=1024, group_cap=C)
    history = []
    for w, (G, n) in enumerate(zip(groups, sizes)):
        recs = sc.identify(sc.window(rng, n, G, C, edges=False, skipped=n > 0), rng)
        r = o.results(o.step_records(recs, G), C)
        n_want, rows = sc.brute_window(recs, G, C, K)
        history.append((rows, np.minimum(n_want, K)))
        k_recent, recent = sc.brute_recent(history, C, K, H)
        np.testing.assert_array_equal(r["k_recent"], k_recent, err_msg=f"step {w}")
        sc.same_rows(r["recent"], recent, f"step {w}")
        res = o.resident()
        assert res["rows"].shape == (H, C, K) and res["k"].shape == (H, C)
        sc.same_rows(res["rows"][w % H], rows, f"step {w} slot")
    assert not history[1][1].any() and not history[2][1].any()  # the empty step, and n_groups = 0
    # groups 2..5 were last present at step 3: gone from the horizon after steps 4, 5, 6
    r6 = o.results(6, C)
    assert not r6["k_recent"][2:].any() and r6["k_recent"][:2].all()
    assert not np.ascontiguousarray(r6["recent"][2:]).view(np.uint8).any()
    assert o.results(7, C)["k_recent"][2:].any()


def test_every_configuration_check_and_every_refused_step():
    good = dict(k=3, windows=3, span_cap=16, group_cap=2, n_buffers=2)
    for kw in (dict(k=0), dict(k=9), dict(windows=0), dict(windows=17), dict(group_cap=0), dict(group_cap=65537),
               dict(span_cap=0), dict(span_cap=1 << 31), dict(n_buffers=0), dict(n_buffers=65)):
        with pytest.raises(ValueError, match="request exemplars"):
            ex.ExemplarOracle(**{**good, **kw})
    # the largest shape the ranges allow stays below the 2 GiB of device rows the last check bounds
    ex.check_config(8, 16, (1 << 31) - 1, 65536, 64)
    assert (16 + 2) * 65536 * 8 * ex.ROW_BYTES <= 1 << 31
    o = ex.ExemplarOracle(span_cap=4, k=2, windows=2, group_cap=2, n_buffers=2)
    with pytest.raises(ValueError, match="n_groups"):
        o.step_records(np.zeros(0, R.SPAN), 3)
    with pytest.raises(ValueError, match="n_groups"):
        o.step_records(np.zeros(0, R.SPAN), -1)
    with pytest.raises(ValueError, match="span_cap"):
        o.step_records(np.zeros(5, R.SPAN), 2)
    with pytest.raises(ValueError, match="whole"):
        o.step([(1 << 20, 63)], 2)
    assert o.n == 0 and not o.resident()["k"].any()  # a refused step is no step
    for i in range(3):
        assert o.step_records(sc.spans([100.0 * (i + 1)], [1]), 2) == i
    assert set(o.results(2, 2)) == set(ex.RESULT_FIELDS)
    assert o.results(2, 2)["n"].tolist() == [0, 1] and o.results(1, 1)["win"].shape == (1, 2)
    assert _ttfts(o.results(2, 2)["recent"][1]) == [300.0, 200.0]
    for i in (0, 3):
        with pytest.raises(IndexError):
            o.results(i, 2)
    assert set(ex.empty_result(3, 2)) == set(ex.RESULT_FIELDS) and ex.empty_result(3, 2)["win"].shape == (3, 2)


# ---- the window pipeline ---------------------------------------------------------------------------

RESULT_KEYS = {"post", "conf", "feat", "pred", "evbits", "sli", "app", "late"}


def test_pipeline_on_the_host_engine_carries_the_new_keys_only_when_switched_on():
    from llm_slo_ebpf_toolkit_amd.pipeline.window import WindowPipeline

    rng = np.random.default_rng(7)
    G, K = 3, 3
    wins = [sc.identify(sc.window(rng, int(n), G, 8, edges=False), rng) for n in rng.integers(0, 60, 6)]
    off, none = sc.run_pipeline("cpu", wins, G, 0)
    on, exs = sc.run_pipeline("cpu", wins, G, K)
    ref = ex.ExemplarOracle(k=K, windows=3, span_cap=1024, group_cap=8)
    assert none == []
    for w, (a, b, s) in enumerate(zip(off, on, exs)):
        assert set(a) == RESULT_KEYS, "exemplars off: today's keys"
        assert set(b) == RESULT_KEYS | set(ex.RESULT_KEYS)
        for key in RESULT_KEYS:
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"window {w} {key}")
        want = ref.results(ref.step_records(wins[w], G), G)
        sc.same_results(s, want, f"window {w}")
        keyed = ex.result_keys(want)
        for key in ("ex_n", "ex_k_win", "ex_k_recent"):
            np.testing.assert_array_equal(b[key], keyed[key], err_msg=f"window {w} {key}")
        sc.same_rows(b["ex_win"], keyed["ex_win"], f"window {w}")
        sc.same_rows(b["ex_recent"], keyed["ex_recent"], f"window {w}")
        np.testing.assert_array_equal(b["ex_n"], b["sli"][:, 0] + b["late"][:, 0], err_msg=f"window {w}")
    assert sum(int(r["ex_n"].sum()) for r in on) > 50
    # one GPU only: a shard of a node's stream is refused, in the sketch's wording
    with pytest.raises(ValueError, match="one GPU: no communicator, no sharding"):
        WindowPipeline(1024, 64, 4, engine="cpu", shard=(0, 2), exemplars=3)
    with pytest.raises(ValueError, match="request exemplars: k"):
        WindowPipeline(1024, 64, 4, engine="cpu", exemplars=9)


# ---- the agent ----------------------------------------------------------------------------------------

def _agent(tmp_path, tag, **kw):
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions

    log = tmp_path / f"decisions-{tag}.jsonl"
    o = AgentOptions(engine="cpu", source="replay", gpus=1, window_events=2048, window_spans=128, window_groups=8,
                     window_ms=300, metrics_bind="", output="stdout", ring_name=f"/mislo-ex-{tag}-{os.getpid()}",
                     config="", min_confidence=0.0, scenario="full", disable_overhead_guard=True,
                     decision_log=str(log), **kw)
    out = io.StringIO()
    a = Agent(o, out_stream=out)
    seen = []
    inner = a._attributions

    def spy(G, names, res, t_ns, model):
        attrs = inner(G, names, res, t_ns, model)
        seen.append((res, attrs))
        return attrs

    a._attributions = spy
    try:
        assert a.run_windows(max_windows=4) == 0
    finally:
        a.close()
    return a, seen, [json.loads(ln) for ln in log.read_text().splitlines()], out.getvalue()


def test_agent_flags_and_the_one_gpu_rule():
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions
    from llm_slo_ebpf_toolkit_amd.cli.agent import parse

    o, _ = parse(["--engine", "cpu", "--request-exemplars", "5", "--exemplar-windows", "2"])
    assert o.request_exemplars == 5 and o.exemplar_windows == 2
    d = parse([])[0]
    assert d.request_exemplars == 0 and d.exemplar_windows == 3 and AgentOptions().request_exemplars == 0
    a = Agent(AgentOptions(engine="cpu", source="replay", config="", output="stdout", metrics_bind="", gpus=2,
                           ring_name=f"/mislo-ex2-{os.getpid()}", request_exemplars=3))
    try:
        with pytest.raises(ValueError, match="one GPU"):
            a.run_windows(max_windows=1)
    finally:
        a.close()


@pytest.mark.timeout(120)
def test_an_emitted_incident_names_the_breaching_requests_and_the_decision_log_lists_them(tmp_path):
    from llm_slo_ebpf_toolkit_amd.contracts import validator
    from llm_slo_ebpf_toolkit_amd.export.prometheus import parse_exposition

    a, seen, rows, out = _agent(tmp_path, "on", request_exemplars=3, exemplar_windows=3)
    slo = F32(a.o.ttft_slo_ms)
    named = 0
    for res, attrs in seen:
        assert set(ex.RESULT_KEYS) <= set(res)
        for attr in attrs:
            g = int(attr.incident_id.rsplit("-", 1)[1])
            rec = res["ex_recent"][g][:int(res["ex_k_recent"][g])]
            bad = rec[rec["ttft_ms"] > slo]
            assert attr.request_ids == [f"{int(s):016x}" for s in bad["span_h"]]
            assert attr.trace_ids == list(dict.fromkeys(f"{int(t):016x}" for t in bad["trace_h"]))
            d = attr.to_dict()
            assert ("request_ids" in d) == ("trace_ids" in d) == bool(len(bad))
            validator.validate("incident-attribution", d)
            named += bool(len(bad))
    assert named > 0, "a window whose group breaches names its requests"
    emitted = [json.loads(ln) for ln in out.splitlines() if ln.startswith('{"incident_id"')]
    assert sum("request_ids" in d for d in emitted) == named
    # the decision log: every scored group's recent exemplars, worst first
    assert rows and all("exemplars" in r for r in rows)
    fields = {"trace_id", "span_id", "ttft_ms", "latency_ms", "retrieval_ms", "pod_id", "pid", "age"}
    busy = [r for r in rows if r["exemplars"]]
    assert busy and all(set(e) == fields for r in busy for e in r["exemplars"])
    for r in busy:
        t = [e["ttft_ms"] for e in r["exemplars"]]
        assert t == sorted(t, reverse=True) and len(t) <= 3 and all(0 <= e["age"] < 3 for e in r["exemplars"])
        assert all(len(e["span_id"]) == 16 and int(e["span_id"], 16) for e in r["exemplars"])
    res, _ = seen[-1]
    g = int(np.argmax(res["ex_k_win"] > 0))
    m = parse_exposition(a.metrics.registry.exposition())
    assert m[f'llm_slo_agent_ttft_max_ms{{service="svc-{g + 1}"}}'] == pytest.approx(float(res["ex_win"][g][0]["ttft_ms"]))
    for reason in ex.EVENT_STATS:
        assert m[f'llm_slo_agent_exemplar_events_total{{reason="{reason}"}}'] == 0
    assert " # {" not in a.metrics.registry.exposition()  # no OpenMetrics exemplar syntax


@pytest.mark.timeout(120)
def test_with_the_flag_off_incidents_and_log_lines_carry_nothing_new(tmp_path):
    a, seen, rows, out = _agent(tmp_path, "off")
    assert seen and all(not set(ex.RESULT_KEYS) & set(res) for res, _ in seen)
    emitted = [json.loads(ln) for ln in out.splitlines() if ln.startswith('{"incident_id"')]
    assert emitted and not any("request_ids" in d or "trace_ids" in d for d in emitted)
    assert set(emitted[0]) == {"incident_id", "timestamp", "cluster", "namespace", "service", "predicted_fault_domain",
                               "confidence", "evidence", "slo_impact", "fault_hypotheses"}
    assert rows and set(rows[0]) == {"t_ns", "group", "service", "requests", "breaches", "burn_now", "burn_forecast",
                                     "top", "late", "emitted", "why"}
    # the same stream with the flag on: the incidents differ by the two id lists alone, the log by its field
    _b, _seen, rows_on, out_on = _agent(tmp_path, "on2", request_exemplars=2)
    on = [json.loads(ln) for ln in out_on.splitlines() if ln.startswith('{"incident_id"')]
    assert len(on) == len(emitted) and len(rows_on) == len(rows)

    def plain(d, drop):
        return {k: v for k, v in d.items() if k not in drop and k not in ("incident_id", "timestamp", "t_ns")}

    for x, y in zip(emitted, on):
        assert plain(x, ()) == plain(y, ("request_ids", "trace_ids"))
    for x, y in zip(rows, rows_on):
        assert plain(x, ()) == plain(y, ("exemplars",))


def test_exemplar_metrics():
    from llm_slo_ebpf_toolkit_amd.agent.metrics import AgentMetrics
    from llm_slo_ebpf_toolkit_amd.export.prometheus import parse_exposition

    o = ex.ExemplarOracle(k=2, windows=2, span_cap=64, group_cap=2)
    m = AgentMetrics("probe", "auto", [], [])
    for vals, grp in (([40.0, 2500.0, 900.0, float("nan")], [0, 0, 0, 0]), ([60.0, 75.0], [0, 5])):
        r = o.results(o.step_records(sc.spans(vals, grp), 2), 2)
        m.observe_exemplars(ex.result_keys(r), ex.stats_dict(r["stats"]), ["rag"])
    v = parse_exposition(m.registry.exposition())
    assert v['llm_slo_agent_ttft_max_ms{service="rag"}'] == 60.0  # the last window's, exact
    assert not any(k.startswith('llm_slo_agent_ttft_max_ms{service="group-1"') for k in v)  # never a NaN
    assert v['llm_slo_agent_exemplar_events_total{reason="invalid"}'] == 1
    assert v['llm_slo_agent_exemplar_events_total{reason="out_of_group"}'] == 1


# ---- the span mapper's trace-id memory -----------------------------------------------------------------

def _otlp_span(trace_id, span_id, ttft=900.0):
    return ({"service.name": "rag"}, {"traceId": trace_id, "spanId": span_id, "startTimeUnixNano": 10 ** 18,
                                      "endTimeUnixNano": 10 ** 18 + 10 ** 9, "attrs": {"llm.ttft_ms": ttft}})


def test_mapper_remembers_the_trace_ids_high_half_bounded_and_only_when_asked():
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent
    from llm_slo_ebpf_toolkit_amd.collector import otlp

    assert otlp.trace_high_half("0af7651916cd43dd8448eb211c80319c") == 0x0AF7651916CD43DD
    assert otlp.trace_high_half(bytes.fromhex("0af7651916cd43dd8448eb211c80319c")) == 0x0AF7651916CD43DD
    assert otlp.trace_high_half("8448eb211c80319c") is None and otlp.trace_high_half(None) is None
    assert otlp.trace_high_half("zz" * 16) is None
    mk = lambda: otlp.SpanMapper(otlp.GroupTable(4), lambda uid: 1)  # noqa: E731
    tid = "0af7651916cd43dd8448eb211c80319c"
    lo = otlp.trace_hash(tid)
    off = mk()
    recs = off.records([_otlp_span(tid, "00f067aa0ba902b7")])
    assert len(recs) == 1 and int(recs["trace_h"][0]) == lo and int(recs["span_h"][0]) == 0x00F067AA0BA902B7
    assert off.trace_high(lo) is None and not off._high, "off: nothing is kept"
    on = mk()
    on.keep_trace_high = True
    on.retrieval_cap = 4
    on.records([_otlp_span(tid, "00f067aa0ba902b7")])
    assert on.trace_high(lo) == 0x0AF7651916CD43DD
    for i in range(1, 5):
        on.records([_otlp_span(f"{i:016x}{i + 100:016x}", f"{i:016x}")])
    assert len(on._high) == 4 and on.trace_high(lo) is None and on.trace_high(104) == 4  # oldest out

    class Stub:  # the daemon's formatting: 32 hex digits with the high half, else the low 16
        mapper = on

    assert Agent._trace_id(Stub(), 104) == f"{4:016x}{104:016x}"
    assert Agent._trace_id(Stub(), lo) == f"{lo:016x}" and len(Agent._trace_id(Stub(), lo)) == 16
    Stub.mapper = None
    assert Agent._trace_id(Stub(), 104) == f"{104:016x}"


# ---- the tracker's host side under the host sanitizers ------------------------------------------------

@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="needs g++")
@pytest.mark.timeout(300)
def test_exemplar_host_side_under_address_and_ub_sanitizers(tmp_path):
    """ops/csrc/exemplars_host.h (order keys, row, argument checks, result layout) needs no device: a
    stand-alone program over it, built with AddressSanitizer + UBSan."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "llm_slo_ebpf_toolkit_amd", "ops", "csrc")
    exe = tmp_path / "exemplars_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-Wall", "-Werror", f"-I{csrc}", os.path.join(root, "tests", "native", "exemplars_host_check.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "exemplars host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
