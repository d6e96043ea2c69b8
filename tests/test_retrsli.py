"""The TTFT phase split's rules on the host (pipeline/retrsli.py): the numpy oracle against a per-record loop on
every named case (tests/retrsli_scenarios.py CASES), every refusal and configuration check, the host engine's
result keys, the agent's flags, decision-log entry and series, and the tracker's host side
(ops/csrc/retrsli_host.h) under the host sanitizers, its answers compared with the same brute force. The device
tracker against the oracle: tests/test_retrsli_gpu.py."""

import io
import json
import os
import struct

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.pipeline import retrsli as rs
from tests import retrsli_scenarios as sc


def test_units_cells_and_states_of_the_oracle_are_the_brute_force_s():
    rng = np.random.default_rng(2)
    ms = np.concatenate([rng.lognormal(np.log(100.0), 3.0, 2000), [0.125, 0.375, 0.625, 0.0, 1e7, np.inf, 167772.14, 167772.16]]).astype(np.float32)
    assert rs.units_of_ms(ms).tolist() == [sc.brute_units(x) for x in ms]
    assert int(rs.units_of_ms(np.float32(sc.SLO))) == sc.SLO_U and rs.budget_units(sc.BUDGET) == sc.BUDGET_U
    assert (rs.budget_units(1e-9), rs.budget_units(0.125), rs.budget_units(1e12)) == (1, 12, rs.UNIT_MAX)
    for tb in (False, True):
        for r in (0, sc.BUDGET_U, sc.BUDGET_U + 1, rs.UNIT_MAX):
            for m in (0, sc.SLO_U, sc.SLO_U + 1, rs.UNIT_MAX):
                assert int(rs.cell_of(tb, r, m, sc.SLO_U, sc.BUDGET_U)) == sc.brute_cell(tb, r, m, sc.SLO_U, sc.BUDGET_U)
    for c, (r, t) in enumerate(sc.CELL_RT):
        assert sc.brute_cell(t > sc.SLO_U, r, t - r, sc.SLO_U, sc.BUDGET_U) == c
    for _ in range(500):
        c = rng.integers(0, 30, 6).tolist()
        args = (int(rng.integers(0, 200)), int(rng.integers(1, 60)), int(rng.integers(0, 10 ** 6 + 1)),
                int(rng.integers(1, 10 ** 6)), int(rng.integers(500_001, 10 ** 6 + 1)))
        assert rs.state_of(c, *args) == sc.brute_state(c, *args)
    assert (rs.age_of(2, 2, 7), rs.age_of(2, 3, 7), rs.age_of(1, 1, 0xFFFFFFFF)) == (8, 1, 0xFFFFFFFF)
    assert rs.budget_ppm(0.99) == 10000 and rs.K == 336 and len(rs.CELLS) == rs.N_CELLS == 6 and len(rs.STATES) == 5


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_oracle_equals_the_per_record_loop_after_every_step(name):
    c = sc.case(name)
    o, brute = rs.RetrievalSliOracle(**c.cfg), sc.Brute(**c.cfg)
    assert (o.slo_units, o.budget_units) == (brute.slo_u, brute.budget_u) == (sc.SLO_U, sc.BUDGET_U)
    C = c.cfg["group_cap"]
    seen = []
    for w, (recs, G) in enumerate(c.steps):
        want = brute.step(recs, G)
        got = o.results(o.step_records(recs, G), C)
        sc.same_results(got, want, f"{name} step {w}")
        sc.same_resident(o.resident(), brute.resident(), f"{name} step {w}", pos=False)
        assert o.resident()["pos"] == (w + 1) % c.cfg["windows"]
        for f in rs.RESULT_FIELDS[:-1]:
            np.testing.assert_array_equal(o.results(w, G)[f], want[f][:G], err_msg=f"{name} step {w} first G rows of {f}")
        blk, off = o.block(w), rs.layout(C)
        assert blk.dtype == np.uint32 and len(blk) == off["words"] and all(v % 4 == 0 for v in off.values())
        np.testing.assert_array_equal(blk[off["sum_t"]:off["sum_t"] + 2 * C].view(np.uint64), want["sum_t"])
        np.testing.assert_array_equal(blk[off["cells_roll"]:off["cells_roll"] + 8 * C].reshape(C, 8)[:, :6], want["cells_roll"])
        assert not blk[off["cells"]:off["cells"] + 8 * C].reshape(C, 8)[:, 6:].any()
        np.testing.assert_array_equal(blk[off["q_m_roll"]:off["q_m_roll"] + 4 * C].reshape(C, 4), want["q_m_roll"])
        np.testing.assert_array_equal(blk[off["age"]:off["age"] + C], want["age"])
        seen.append(got)
    if c.check is not None:
        c.check(seen)


BAD_CONFIGS = ((dict(windows=0), "windows"), (dict(windows=4097), "windows"), (dict(group_cap=0), "group_cap"),
               (dict(group_cap=65537), "group_cap"), (dict(span_cap=0), "span_cap"), (dict(n_buffers=0), "n_buffers"),
               (dict(n_buffers=65), "n_buffers"), (dict(slo_ms=-1.0), "slo_ms"), (dict(slo_ms=float("nan")), "slo_ms"),
               (dict(slo_ms=float("inf")), "slo_ms"), (dict(retrieval_budget_ms=0.0), "retrieval_budget_ms"),
               (dict(retrieval_budget_ms=-1.0), "retrieval_budget_ms"), (dict(retrieval_budget_ms=float("nan")), "retrieval_budget_ms"),
               (dict(retrieval_budget_ms=float("inf")), "retrieval_budget_ms"), (dict(budget_ppm=0), "budget_ppm"),
               (dict(budget_ppm=1_000_000), "budget_ppm"), (dict(coverage_ppm=-1), "coverage_ppm"),
               (dict(coverage_ppm=1_000_001), "coverage_ppm"), (dict(dominance_ppm=500_000), "dominance_ppm"),
               (dict(dominance_ppm=1_000_001), "dominance_ppm"), (dict(min_requests=0), "min_requests"),
               (dict(min_requests=1 << 31), "min_requests"), (dict(span_cap=1 << 21, windows=2048), "below 2"),
               (dict(group_cap=65536, windows=4096), "2 GiB"))


def test_every_configuration_check_and_every_refused_step():
    for kw, msg in BAD_CONFIGS:
        with pytest.raises(ValueError, match=msg):
            rs.RetrievalSliOracle(**kw)
    rs.RetrievalSliOracle(windows=1, group_cap=1, span_cap=1, n_buffers=1, slo_ms=0.0, retrieval_budget_ms=1e-9, budget_ppm=1,
                          coverage_ppm=0, dominance_ppm=500_001, min_requests=1).close()
    rs.RetrievalSliOracle(budget_ppm=999_999, coverage_ppm=1_000_000, dominance_ppm=1_000_000, min_requests=(1 << 31) - 1).close()
    rng = np.random.default_rng(5)
    recs = np.ascontiguousarray(sc.mixed_window(rng, 50, 3))
    o = rs.RetrievalSliOracle(**sc._cfg(span_cap=len(recs)))
    o.step_records(recs, 3)
    before = {k: np.array(v, copy=True) for k, v in o.resident().items()}
    a = recs.ctypes.data
    for bad in (lambda: o.step([(a, 63)], 3), lambda: o.step([(0, 64)], 3), lambda: o.step_records(recs, 5),
                lambda: o.step_records(recs, -1), lambda: o.step_records(np.concatenate([recs, recs[:1]]), 3)):
        with pytest.raises(ValueError, match="retrieval sli step"):
            bad()
    sc.same_resident(o.resident(), before, "a refused step changes nothing")
    assert o.step([(a, 64 * 10), (a + 640, 0), (a + 640, 64 * 5)], 3) == 1
    brute = sc.Brute(**sc._cfg())
    brute.step(recs, 3)
    sc.same_results(o.results(1, 4), brute.step(recs[:15], 3), "the step after the refused ones")
    with pytest.raises(IndexError):
        o.results(5, 3)


# ---- the pipeline -------------------------------------------------------------------------------------

def test_pipeline_on_the_host_engine_carries_the_new_keys_only_when_switched_on():
    from llm_slo_ebpf_toolkit_amd.pipeline.window import WindowPipeline

    rng = np.random.default_rng(41)
    groups = [3, 3, 2, 3]
    wins = [sc.mixed_window(rng, 40, 3) if w != 2 else np.zeros(0, R.SPAN) for w in range(4)]
    off, none = sc.run_pipeline("cpu", wins, groups, 0)
    onr, ret = sc.run_pipeline("cpu", wins, groups, 2)
    ref = rs.RetrievalSliOracle(**sc._cfg(group_cap=8, windows=2))
    assert none == []
    for w, (a, b, d) in enumerate(zip(off, onr, ret)):
        assert not any(k.startswith("retr_") for k in a) and set(b) == set(a) | set(rs.RESULT_KEYS)
        assert all(k.startswith("retr_") for k in rs.RESULT_KEYS)
        for key in a:  # the existing keys: byte-equal with the tracker on and off
            assert np.ascontiguousarray(a[key]).tobytes() == np.ascontiguousarray(b[key]).tobytes(), f"window {w} {key}"
        want = ref.results(ref.step_records(wins[w], groups[w]), groups[w])
        sc.same_results(d, want, f"window {w}")
        for key, v in rs.result_keys(want).items():
            np.testing.assert_array_equal(b[key], v, err_msg=f"window {w} {key}")
    assert np.isnan(onr[0]["retr_q"]).sum() == 0 and int(onr[2]["retr_cells"].sum()) == 0 and np.isnan(onr[2]["retr_model_q"]).all()
    assert int(onr[1]["retr_cells_roll"].sum()) > int(onr[1]["retr_cells"].sum()) > 20
    with pytest.raises(ValueError, match="one GPU: no communicator, no sharding"):
        WindowPipeline(1024, 64, 4, engine="cpu", shard=(0, 2), retrieval_sli=2)
    with pytest.raises(ValueError, match="retrieval sli: retrieval_budget_ms"):
        WindowPipeline(1024, 64, 4, engine="cpu", retrieval_sli=2, retr_budget_ms=0.0)
    with pytest.raises(ValueError, match="retrieval sli: windows"):
        WindowPipeline(1024, 64, 4, engine="cpu", retrieval_sli=5000)
    with pytest.raises(ValueError, match="retrieval sli: dominance_ppm"):
        WindowPipeline(1024, 64, 4, engine="cpu", retrieval_sli=2, retr_dominance_ppm=500_000)
    p = WindowPipeline(1024, 64, 4, engine="cpu", ttft_slo_ms=1000.0, retrieval_sli=2)
    try:
        assert p.retr.budget_units == 25_000  # a quarter of the SLO
    finally:
        p.close()
    p = WindowPipeline(1024, 64, 4, engine="cpu")
    try:
        assert p.retr is None
    finally:
        p.close()


# ---- the agent ----------------------------------------------------------------------------------------

def _agent(tmp_path, tag, **kw):
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions

    log = tmp_path / f"decisions-{tag}.jsonl"
    o = AgentOptions(engine="cpu", source="replay", gpus=1, window_events=2048, window_spans=128, window_groups=8,
                     window_ms=300, metrics_bind="", output="stdout", ring_name=f"/mislo-rs-{tag}-{os.getpid()}",
                     config="", min_confidence=0.0, scenario="full", disable_overhead_guard=True,
                     decision_log=str(log), **kw)
    out = io.StringIO()
    a = Agent(o, out_stream=out)
    try:
        assert a.run_windows(max_windows=4) == 0
    finally:
        a.close()
    return a, [json.loads(ln) for ln in log.read_text().splitlines()], out.getvalue()


def test_agent_flags_defaults_and_the_one_gpu_rule():
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions
    from llm_slo_ebpf_toolkit_amd.cli.agent import parse

    o, _ = parse(["--engine", "cpu", "--retrieval-sli", "--retrieval-budget-ms", "150", "--retrieval-horizon-windows", "30",
                  "--retrieval-min-requests", "50", "--retrieval-min-coverage", "0.25", "--retrieval-dominance", "0.8"])
    assert (o.retrieval_sli, o.retrieval_budget_ms, o.retrieval_horizon_windows, o.retrieval_min_requests,
            o.retrieval_min_coverage, o.retrieval_dominance) == (True, 150.0, 30, 50, 0.25, 0.8)
    d = parse([])[0]
    assert (d.retrieval_sli, d.retrieval_budget_ms, d.retrieval_horizon_windows, d.retrieval_min_requests,
            d.retrieval_min_coverage, d.retrieval_dominance) == (False, 0.0, 0, 200, 0.5, 0.667)
    assert AgentOptions().retrieval_sli is False
    kw = dict(engine="cpu", source="replay", config="", output="stdout", metrics_bind="")
    a = Agent(AgentOptions(ring_name=f"/mislo-rs2-{os.getpid()}", window_ms=2000, ttft_horizon_windows=40, ttft_slo_ms=1000.0,
                           slo_target=0.95, **kw))
    try:
        assert a.retrieval_horizon() == a.ttft_horizon() == 40  # the sketch's by default
        assert a.retrieval_budget_ms() == 250.0  # a quarter of the SLO
        assert a.retrieval_params() == dict(budget_ppm=50_000, coverage_ppm=500_000, dominance_ppm=667_000, min_requests=200)
        a.check_retrieval_flags()
    finally:
        a.close()
    a = Agent(AgentOptions(ring_name=f"/mislo-rs3-{os.getpid()}", window_ms=2000, retrieval_horizon_windows=7,
                           retrieval_budget_ms=90.0, retrieval_dominance=0.5, **kw))
    try:
        assert a.retrieval_horizon() == 7 and a.ttft_horizon() == 150 and a.retrieval_budget_ms() == 90.0
        with pytest.raises(ValueError, match="dominance_ppm.*--retrieval-dominance"):
            a.check_retrieval_flags()
    finally:
        a.close()
    for bad in (dict(retrieval_budget_ms=-1.0), dict(retrieval_min_requests=0), dict(retrieval_min_coverage=1.5),
                dict(retrieval_horizon_windows=5000)):
        a = Agent(AgentOptions(ring_name=f"/mislo-rs5-{os.getpid()}", retrieval_sli=True, **bad, **kw))
        try:
            with pytest.raises(ValueError, match="--retrieval-"):
                a.run_windows(max_windows=1)
        finally:
            a.close()
    a = Agent(AgentOptions(gpus=2, ring_name=f"/mislo-rs4-{os.getpid()}", retrieval_sli=True, **kw))
    try:
        with pytest.raises(ValueError, match="--retrieval-sli runs on one GPU"):
            a.run_windows(max_windows=1)
    finally:
        a.close()


PHASES = {"ok", "ok_slow_retrieval", "model", "model_slow_retrieval", "retrieval", "combined"}
TIMES = {"p50", "p90", "p95", "p99", "mean"}
SUMMARY = {"requests", "coverage", "share", "phases", "retrieval_ms", "model_ms"}


def _entry_shape(e):
    assert set(e) == SUMMARY | {"state", "age_windows", "horizon"} and set(e["horizon"]) == SUMMARY
    for s in (e, e["horizon"]):
        assert set(s["phases"]) == PHASES and set(s["retrieval_ms"]) == set(s["model_ms"]) == TIMES
    assert e["state"] in rs.STATES


def test_the_decision_log_entry_and_the_series_from_a_fabricated_result():
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent
    from llm_slo_ebpf_toolkit_amd.agent.metrics import AgentMetrics
    from llm_slo_ebpf_toolkit_amd.export.prometheus import parse_exposition

    o = rs.RetrievalSliOracle(**sc._cfg(group_cap=3, windows=2))
    o.step_records(sc.by_cells(1, [8, 0, 0, 0, 0, 0]), 3)
    i = o.step_records(np.concatenate([sc.by_cells(1, [1, 0, 1, 0, 2, 0], no_breakdown=4), sc.by_cells(2, [0, 0, 0, 1, 0, 0])]), 3)
    res = rs.result_keys(o.results(i, 3))
    e = [Agent._retrieval_entry(res, g) for g in range(3)]
    for x in e:
        _entry_shape(x)
    empty = {"requests": 0, "coverage": None, "share": None, "phases": dict.fromkeys(rs.CELLS, 0),
             "retrieval_ms": dict.fromkeys(TIMES), "model_ms": dict.fromkeys(TIMES)}
    assert e[0] == {"state": "unknown", "age_windows": 2, **empty, "horizon": empty}
    assert e[1]["requests"] == 4 and e[1]["coverage"] == 0.5 and e[1]["phases"] == dict(zip(rs.CELLS, [1, 0, 1, 0, 2, 0]))
    sum_r, sum_t = 100 + 100 + 2 * 30_000, 1_000 + 90_000 + 2 * 90_000
    assert e[1]["share"] == round(sum_r / sum_t, 6) and e[1]["retrieval_ms"]["mean"] == round(sum_r / 100 / 4, 4)
    assert e[1]["model_ms"]["mean"] == round((sum_t - sum_r) / 100 / 4, 4)
    rep = rs.representative() / 100.0
    assert e[1]["retrieval_ms"]["p50"] == round(float(rep[sc.bucket(100)]), 4)
    assert e[1]["retrieval_ms"]["p99"] == round(float(rep[sc.bucket(30_000)]), 4)
    assert abs(e[1]["retrieval_ms"]["p99"] - 300.0) <= 300.0 / 32 and e[1]["model_ms"]["p99"] == round(float(rep[sc.bucket(89_900)]), 4)
    h = e[1]["horizon"]
    # 12 requests, 3 breaches of them (budget 1/10), 2 of the 3 by retrieval: below the dominance of 3/4
    assert h["requests"] == 12 and h["coverage"] == 0.75 and h["phases"]["ok"] == 9 and (e[1]["state"], e[1]["age_windows"]) == ("mixed", 1)
    assert e[2]["state"] == "unknown" and e[2]["phases"]["model_slow_retrieval"] == 1 and e[2]["share"] == 0.25
    json.dumps(e)
    m = AgentMetrics("probe", "auto", [], [])
    stats = {"observed": 5, "out_of_group": 1, "invalid": 2, "no_breakdown": 4, "extra": 3, "exceeds_ttft": 6}
    m.observe_retrieval(res, stats, ["rag", "chat"])
    m.observe_retrieval(res, stats, ["rag", "chat"])
    text = m.registry.exposition()
    v = parse_exposition(text)
    assert v['llm_slo_agent_ttft_phase_state{service="chat"}'] == 4 and v['llm_slo_agent_ttft_phase_state{service="rag"}'] == 0
    assert v['llm_slo_agent_ttft_phase_state{service="group-2"}'] == 0
    assert v['llm_slo_agent_retrieval_share{service="group-2"}'] == pytest.approx(0.25)
    assert 'llm_slo_agent_retrieval_share{service="rag"}' not in text, "no request: no series"
    assert 'llm_slo_agent_retrieval_ms{service="rag"' not in text and 'llm_slo_agent_model_ttft_ms{service="rag"' not in text
    assert v['llm_slo_agent_retrieval_ms{service="chat",quantile="0.5"}'] == pytest.approx(float(rep[sc.bucket(100)]))
    assert v['llm_slo_agent_retrieval_ms{service="chat",quantile="0.99"}'] == pytest.approx(float(rep[sc.bucket(30_000)]))
    assert v['llm_slo_agent_model_ttft_ms{service="chat",quantile="0.99"}'] == pytest.approx(float(rep[sc.bucket(89_900)]))
    assert v['llm_slo_agent_model_ttft_ms{service="group-2",quantile="0.9"}'] == pytest.approx(float(rep[sc.bucket(90_000)]))
    for phase, n in zip(rs.CELLS, (1, 0, 1, 0, 2, 0)):
        key = f'llm_slo_agent_ttft_breach_phase_total{{service="chat",phase="{phase}"}}'
        assert (v[key] == 2 * n) if n else (key not in text)
    for reason in rs.EVENT_STATS:
        assert v[f'llm_slo_agent_retrieval_events_total{{reason="{reason}"}}'] == 2 * stats[reason]
    assert set(rs.EVENT_STATS) == {"out_of_group", "invalid", "no_breakdown", "extra", "exceeds_ttft"}


@pytest.mark.timeout(120)
def test_the_agent_logs_a_retrieval_entry_per_scored_group_and_off_means_nothing_new(tmp_path):
    from llm_slo_ebpf_toolkit_amd.contracts import validator

    a, rows, out = _agent(tmp_path, "on", retrieval_sli=True, retrieval_horizon_windows=3)
    assert rows and all("retrieval" in r for r in rows)
    for r in rows:
        _entry_shape(r["retrieval"])
    spec = a.specs[0]
    assert spec.retrieval_sli == 3 and spec.retr_budget_ms == 200.0
    assert dict(spec.retr_params) == dict(budget_ppm=10_000, coverage_ppm=500_000, dominance_ppm=667_000, min_requests=200)
    emitted = [json.loads(ln) for ln in out.splitlines() if ln.startswith('{"incident_id"')]
    assert emitted
    for d in emitted:
        assert "retrieval" not in d
        validator.validate("incident-attribution", d)
    text = a.metrics.registry.exposition()
    assert 'llm_slo_agent_retrieval_events_total{reason="no_breakdown"}' in text and "llm_slo_agent_ttft_phase_state{" in text
    # four windows cannot hold the 200 requests a verdict needs; a group without a breakdown has nulls
    assert all(r["retrieval"]["state"] == "unknown" for r in rows)
    for r in rows:
        e = r["retrieval"]
        if e["requests"] == 0:
            assert e["share"] is None and e["retrieval_ms"]["p50"] is None and e["model_ms"]["mean"] is None
        else:
            assert e["share"] is not None and e["retrieval_ms"]["p50"] is not None and e["coverage"] is not None
    b, rows_off, out_off = _agent(tmp_path, "off")
    assert b.specs[0].retrieval_sli == 0 and all("retrieval" not in r for r in rows_off)
    off_text = b.metrics.registry.exposition()
    assert "llm_slo_agent_retrieval_events_total{" not in off_text and "llm_slo_agent_ttft_phase_state{" not in off_text
    # the replay is cut by the wall clock, so two runs need not see the same windows: the shapes are compared
    off = [json.loads(ln) for ln in out_off.splitlines() if ln.startswith('{"incident_id"')]
    assert off and {frozenset(d) for d in off} == {frozenset(d) for d in emitted}, "emitted incidents keep their fields"
    assert {frozenset(r) | {"retrieval"} for r in rows_off} == {frozenset(r) for r in rows}


# ---- the tracker's host side under the host sanitizers ------------------------------------------------

@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="needs g++")
@pytest.mark.timeout(300)
def test_retrsli_host_side_under_address_and_ub_sanitizers(tmp_path):
    """ops/csrc/retrsli_host.h (the unit conversions, the cell, the verdict and its 64-bit products against
    __int128, the LDS key, argument checks, layout, ranges) needs no device: a stand-alone program over it, built
    with AddressSanitizer + UBSan, run as a child process. It answers a file of questions, which must be the
    brute force's answers, and prints the layout of several group counts, which must be the Python mirror's."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "llm_slo_ebpf_toolkit_amd", "ops", "csrc")
    exe = tmp_path / "retrsli_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-Wall", "-Werror", f"-I{csrc}", os.path.join(root, "tests", "native", "retrsli_host_check.cpp"),
                    "-o", str(exe)], check=True)
    rng = np.random.default_rng(9)
    ms = np.concatenate([rng.lognormal(np.log(100.0), 3.0, 300), [0.125, 0.375, 0.625, 0.0, 799.995, 1e7, np.inf, 167772.14,
                                                                    167772.16]]).astype(np.float32)
    ask, want = [], []
    for x in ms:
        ask.append("u %08x" % struct.unpack("<I", struct.pack("<f", float(x)))[0])
        want.append(f"u {sc.brute_units(x)}")
    for b in (200.0, 1e-9, 0.125, 250.0, 1e12, 37.5):
        ask.append(f"b {b!r}")
        want.append(f"b {min(rs.UNIT_MAX, max(1, int(round(b * 100.0))))}")
    for tb in (0, 1):
        for r in (0, sc.BUDGET_U, sc.BUDGET_U + 1, rs.UNIT_MAX):
            for m in (0, sc.SLO_U, sc.SLO_U + 1, rs.UNIT_MAX):
                ask.append(f"c {tb} {r} {m} {sc.SLO_U} {sc.BUDGET_U}")
                want.append(f"c {sc.brute_cell(bool(tb), r, m, sc.SLO_U, sc.BUDGET_U)}")
    big = (1 << 32) - 1
    rows = [([big, 0, 0, 0, 0, 0], big, 1, 10 ** 6, 1, 10 ** 6), ([0, 0, 0, 0, big, 0], big, (1 << 31) - 1, 10 ** 6, 999_999, 10 ** 6),
            ([0, 0, big - 1, 1, 0, 0], 0, 1, 0, 1, 500_001), ([big - 3, 0, 1, 0, 1, 1], big, 1, 999_999, 1, 750_000)]
    for _ in range(300):
        rows.append((rng.integers(0, 30, 6).tolist(), int(rng.integers(0, 200)), int(rng.integers(1, 60)),
                     int(rng.integers(0, 10 ** 6 + 1)), int(rng.integers(1, 10 ** 6)), int(rng.integers(500_001, 10 ** 6 + 1))))
    for c, *args in rows:
        ask.append("s " + " ".join(str(x) for x in (*c, *args)))
        want.append(f"s {sc.brute_state(c, *args)}")
    questions = tmp_path / "questions.txt"
    questions.write_text("\n".join(ask) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), str(questions)], capture_output=True, text=True, env=env, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "retrsli host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
    got = [ln for ln in r.stdout.splitlines() if ln[:2] in ("u ", "b ", "c ", "s ")]
    assert got == want
    lay = [tuple(int(x) for x in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("layout ")]
    assert len(lay) == 7
    for g, *at in lay:
        off = rs.layout(g)
        assert at == [off[k] for k in (*rs.RESULT_FIELDS, "words")]
