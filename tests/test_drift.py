"""The TTFT drift's rules on the host (pipeline/drift.py): the numpy oracle against a brute force over raw
values on every named case (tests/drift_scenarios.py CASES), the bucket rule (the sketch's), every refusal
including the wrap bound, the host engine's result keys (and byte-equal results with the tracker off), the
other six oracles unaffected, the agent's flags, decision-log entry and series, the emission gate on a seeded
stream whose TTFT median moves 400 -> 520 ms under an 800 ms SLO, and the tracker's host side
(ops/csrc/drift_host.h) under the host sanitizers. The device tracker against the oracle:
tests/test_drift_gpu.py."""

import io
import json
import os

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.pipeline import drift as dr
from llm_slo_ebpf_toolkit_amd.pipeline import slisketch as sk
from tests import drift_scenarios as sc


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_oracle_equals_the_brute_force_after_every_step(name):
    c = sc.case(name)
    o, brute = dr.DriftOracle(**c.cfg), sc.Brute(**c.cfg)
    C = c.cfg["group_cap"]
    seen = []
    for w, (recs, G) in enumerate(c.steps):
        want = brute.step(recs, G)
        got = o.results(o.step_records(recs, G), C)
        sc.same_results(got, want, f"{name} step {w}")
        sc.same_resident(o.resident(), brute.resident(), f"{name} step {w}")
        for f in dr.RESULT_FIELDS[:-1]:
            np.testing.assert_array_equal(o.results(w, G)[f], want[f][:G], err_msg=f"{name} step {w} first G rows of {f}")
        blk, off = o.block(w), dr.layout(C)
        assert blk.dtype == np.uint32 and len(blk) == off["words"] and all(v % 4 == 0 for v in off.values())
        np.testing.assert_array_equal(blk[off["slow_num"]:off["slow_num"] + 2 * C].view(np.uint64), want["slow_num"])
        np.testing.assert_array_equal(blk[off["q_base"]:off["q_base"] + 4 * C].reshape(C, 4), want["q_base"])
        np.testing.assert_array_equal(blk[off["state"]:off["state"] + C], want["state"])
        seen.append(got)
    if c.check is not None:
        c.check(seen)


def test_the_bucket_rule_and_the_ranks_are_the_sketch_s():
    assert (dr.K, dr.ROW_STRIDE, dr.EMPTY, dr.PERMILLE) == (sk.K, sk.ROW_STRIDE, sk.EMPTY, sk.PERMILLE) == (386, 392, 0xFFFFFFFF, (500, 900, 950, 990))
    assert dr.bucket_of is sk.bucket_of and dr.rank_buckets is sk.rank_buckets and dr.PER_LANE * 56 == dr.ROW_STRIDE
    for b in range(dr.K):
        for top in (False, True):
            assert int(sk.bucket_of(sc.val(b, top))) == b == sc.brute_bucket(sc.val(b, top)), (b, top)
    # the same window through the sketch's oracle and this one: the window's histograms are the same records
    rng = np.random.default_rng(8)
    recs = sc.mixed_window(rng, 300, 3, [300.0, 500.0, 80.0])
    s = sk.SliSketchOracle(span_cap=1024, group_cap=3, windows=2)
    d = dr.DriftOracle(**sc._cfg(span_cap=1024))
    a, b = s.results(s.step_records(recs, 3), 3), d.results(d.step_records(recs, 3), 3)
    np.testing.assert_array_equal(a["n"], b["n_win"])
    np.testing.assert_array_equal(a["q_win"], b["q_recent"])
    np.testing.assert_array_equal(s.window_hist(), d.resident()["recent"][:, :dr.K])
    assert [int(a["stats"][i]) for i in (0, 1, 4)] == [int(b["stats"][i]) for i in (0, 1, 2)]
    assert dr.defaults(1000.0) == (10, 10, 300) and dr.defaults(250.0) == (40, 40, 1200) and dr.defaults(1e9) == (1, 1, 1)
    o = dr.DriftOracle()
    assert (o.cfg["min_base_windows"], o.cfg["hold_max"], o.cfg["crit"], o.cfg["min_shift"], o.cfg["min_recent"],
            o.cfg["min_base"]) == (10, 1200, 4.0, 2, 30, 100) and o.crit_q == 4 << 32
    assert dr.DriftOracle(baseline=4).cfg["min_base_windows"] == 4


def test_every_configuration_check_and_every_refused_step():
    msgs = ["recent windows", "recent windows", "gap windows", "gap windows", "baseline windows", "baseline windows",
            "group_cap", "group_cap", "span_cap", "slow_num << 16 would wrap", "below 2.44", "n_buffers", "n_buffers",
            "crit", "crit", "crit", "crit", "min_shift", "min_shift", "min_recent", "min_recent", "min_recent", "hold_max",
            "2 GiB"]
    assert len(msgs) == len(sc.BAD_CONFIGS)
    for kw, msg in zip(sc.BAD_CONFIGS, msgs):
        with pytest.raises(ValueError, match=msg):
            dr.DriftOracle(**kw)
    # one below the wrap bound, and the smallest and largest of everything else
    dr.check_config(1 << 16, 1, 64, 1, 63, 1, 4.0, 2, 30, 100, 10, 252)
    dr.DriftOracle(recent=1, gap=1, baseline=1, group_cap=1, span_cap=1, n_buffers=1, crit=1e-12, min_shift=0, hold_max=1).close()
    dr.DriftOracle(recent=1, gap=1, baseline=1, group_cap=1, span_cap=(1 << 22) - 1, n_buffers=64, min_shift=385).close()
    rng = np.random.default_rng(5)
    recs = np.ascontiguousarray(sc.mixed_window(rng, 50, 3, [300.0, 500.0, 80.0]))
    o = dr.DriftOracle(**sc._cfg(span_cap=len(recs)))
    o.step_records(recs, 3)
    before = {k: np.array(v, copy=True) for k, v in o.resident().items()}
    a = recs.ctypes.data
    for bad in (lambda: o.step([(a, 63)], 3), lambda: o.step([(0, 64)], 3), lambda: o.step_records(recs, 4),
                lambda: o.step_records(recs, -1), lambda: o.step_records(np.concatenate([recs, recs[:1]]), 3)):
        with pytest.raises(ValueError, match="ttft drift step"):
            bad()
    sc.same_resident(o.resident(), before, "a refused step changes nothing")
    assert o.step([(a, 64 * 10), (a + 640, 0), (a + 640, 64 * 5)], 3) == 1
    brute = sc.Brute(**sc._cfg())
    brute.step(recs, 3)
    sc.same_results(o.results(1, 3), brute.step(recs[:15], 3), "the step after the refused ones")
    with pytest.raises(IndexError):
        o.results(5, 3)


# ---- the pipeline -------------------------------------------------------------------------------------

def test_pipeline_on_the_host_engine_carries_the_new_keys_only_when_switched_on():
    from llm_slo_ebpf_toolkit_amd.pipeline.window import WindowPipeline

    rng = np.random.default_rng(41)
    groups = [3, 3, 2, 3, 3, 3]
    wins = [sc.mixed_window(rng, 40, 3, [300.0, 500.0, 80.0]) if w != 2 else np.zeros(0, R.SPAN) for w in range(6)]
    kw = dict(drift_min_recent=2, drift_min_base=2, drift_min_base_windows=1, drift_hold_max=3, drift_crit=4.0, drift_min_shift=2)
    off, none = sc.run_pipeline("cpu", wins, groups, None)
    onr, out = sc.run_pipeline("cpu", wins, groups, (2, 1, 3), **kw)
    ref = dr.DriftOracle(**sc._cfg(group_cap=8, span_cap=1024))
    assert none == []
    for w, (a, b, d) in enumerate(zip(off, onr, out)):
        assert not set(a) & set(dr.RESULT_KEYS) and set(b) == set(a) | set(dr.RESULT_KEYS)
        for key in a:  # flag off: byte-equal results
            assert np.ascontiguousarray(a[key]).tobytes() == np.ascontiguousarray(b[key]).tobytes(), f"window {w} {key}"
        want = ref.results(ref.step_records(wins[w], groups[w]), groups[w])
        sc.same_results(d, want, f"window {w}")
        for key, v in dr.result_keys(want).items():
            np.testing.assert_array_equal(b[key], v, err_msg=f"window {w} {key}")
    assert int(onr[2]["drift_n_win"].sum()) == 0 and int(onr[5]["drift_n_base"].sum()) > 0
    with pytest.raises(ValueError, match="one GPU: no communicator, no sharding"):
        WindowPipeline(1024, 64, 4, engine="cpu", shard=(0, 2), ttft_drift=(2, 1, 3))
    with pytest.raises(ValueError, match="ttft drift: crit"):
        WindowPipeline(1024, 64, 4, engine="cpu", ttft_drift=(2, 1, 3), drift_crit=0.0)
    with pytest.raises(ValueError, match="ttft drift: baseline windows"):
        WindowPipeline(1024, 64, 4, engine="cpu", ttft_drift=(2, 1, 5000))
    p = WindowPipeline(1024, 64, 4, engine="cpu")
    try:
        assert p.drift is None
    finally:
        p.close()


def test_the_six_other_oracles_are_unaffected():
    """The drift tracker reads the same span ranges and writes nothing the others read: with it on, every key
    the other six trackers add to the host engine's results is byte-equal."""
    rng = np.random.default_rng(42)
    wins = [sc.mixed_window(rng, 60, 3, [300.0, 900.0, 80.0]) for _ in range(4)]
    for r in wins:
        r["pod_id"] = rng.integers(1, 5, len(r))
    others = dict(open_requests=1 << 10, sli_sketch=2, exemplars=2, pod_breakdown=2, breach_onset=64, decode_sli=2)
    a, _ = sc.run_pipeline("cpu", wins, 3, None, **others)
    b, _ = sc.run_pipeline("cpu", wins, 3, (2, 1, 3), **others)
    seen = set()
    for w, (x, y) in enumerate(zip(a, b)):
        assert set(y) == set(x) | set(dr.RESULT_KEYS)
        for key in x:
            assert np.ascontiguousarray(x[key]).tobytes() == np.ascontiguousarray(y[key]).tobytes(), f"window {w} {key}"
        seen |= set(x)
    assert {"deadline", "ttft_n", "ex_n", "pod_rec_top", "onset_rows", "decode_cells"} <= seen


# ---- the agent ----------------------------------------------------------------------------------------

def _agent(tmp_path, tag, **kw):
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions

    log = tmp_path / f"decisions-{tag}.jsonl"
    o = AgentOptions(engine="cpu", source="replay", gpus=1, window_events=2048, window_spans=128, window_groups=8,
                     window_ms=300, metrics_bind="", output="stdout", ring_name=f"/mislo-dr-{tag}-{os.getpid()}",
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

    o, _ = parse(["--engine", "cpu", "--ttft-drift", "--emit-on-drift", "--drift-recent-windows", "5", "--drift-gap-windows", "6",
                  "--drift-baseline-windows", "70", "--drift-crit", "3.5", "--drift-min-shift-buckets", "3"])
    assert (o.ttft_drift, o.emit_on_drift, o.drift_recent_windows, o.drift_gap_windows, o.drift_baseline_windows, o.drift_crit,
            o.drift_min_shift_buckets) == (True, True, 5, 6, 70, 3.5, 3)
    d = parse([])[0]
    assert (d.ttft_drift, d.emit_on_drift, d.drift_recent_windows, d.drift_gap_windows, d.drift_baseline_windows, d.drift_crit,
            d.drift_min_shift_buckets) == (False, False, 0, 0, 0, 4.0, 2)
    assert AgentOptions().ttft_drift is False and AgentOptions().emit_on_drift is False
    kw = dict(engine="cpu", source="replay", config="", output="stdout", metrics_bind="")
    a = Agent(AgentOptions(ring_name=f"/mislo-dr2-{os.getpid()}", window_ms=2000, drift_gap_windows=7, **kw))
    try:
        assert a.drift_windows() == (5, 7, 150)
    finally:
        a.close()
    a = Agent(AgentOptions(gpus=2, ring_name=f"/mislo-dr3-{os.getpid()}", ttft_drift=True, **kw))
    try:
        with pytest.raises(ValueError, match="--ttft-drift runs on one GPU"):
            a.run_windows(max_windows=1)
    finally:
        a.close()
    a = Agent(AgentOptions(ring_name=f"/mislo-dr4-{os.getpid()}", emit_on_drift=True, **kw))
    try:
        with pytest.raises(ValueError, match="--emit-on-drift needs --ttft-drift"):
            a.run_windows(max_windows=1)
    finally:
        a.close()


def test_the_decision_log_entry_and_the_series_from_a_fabricated_result():
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent
    from llm_slo_ebpf_toolkit_amd.agent.metrics import AgentMetrics
    from llm_slo_ebpf_toolkit_amd.export.prometheus import parse_exposition

    c = sc.case("disjoint rows")   # service 1: baseline 10 records in bucket 100, recent 10 in bucket 200
    o = dr.DriftOracle(**c.cfg)
    for recs, G in c.steps:
        i = o.step_records(recs, G)
    res = dr.result_keys(o.results(i, 3))
    e = [Agent._drift_entry(res, g) for g in range(3)]
    keys = {"state", "distance", "n_recent", "n_base", "p50_ms", "p90_ms", "held_windows"}
    assert all(set(x) == keys for x in e)
    assert e[0] == {"state": "warming", "distance": None, "n_recent": 0, "n_base": 0, "p50_ms": [None, None],
                    "p90_ms": [None, None], "held_windows": 0}
    rep = sk.representative()
    assert e[1] == {"state": "slow", "distance": 1.0, "n_recent": 10, "n_base": 10,
                    "p50_ms": [round(float(rep[100]), 4), round(float(rep[200]), 4)],
                    "p90_ms": [round(float(rep[100]), 4), round(float(rep[200]), 4)], "held_windows": 1}
    json.dumps(e)
    s = dr.summary(res["drift_state"][1], res["drift_hold"][1], 10, 10, 100, res["drift_q_recent"][1], res["drift_q_base"][1])
    assert s["shift_ratio"] == round(float(rep[200]) / float(rep[100]), 6) and s["distance"] == 1.0
    assert [dr.state_name(x) for x in (0, 1, 2, 3, 4, 12)] == ["calm", "slow", "fast", "slow", "warming", "rebased"]
    m = AgentMetrics("probe", "auto", [], [])
    stats = {"observed": 4, "invalid": 1, "out_of_group": 2, "admitted": 3, "withheld": 4, "rebased": 5}
    m.observe_drift(res, stats, ["rag", "chat"])
    m.observe_drift(res, stats, ["rag", "chat"])
    text = m.registry.exposition()
    v = parse_exposition(text)
    assert v['llm_slo_agent_ttft_drift_state{service="rag"}'] == 3 and v['llm_slo_agent_ttft_drift_state{service="chat"}'] == 1
    assert v['llm_slo_agent_ttft_drift_state{service="group-2"}'] == 3
    assert v['llm_slo_agent_ttft_drift_distance{service="chat"}'] == 1.0
    assert v['llm_slo_agent_ttft_drift_shift_ratio{service="chat"}'] == pytest.approx(float(rep[200]) / float(rep[100]), rel=1e-5)
    assert 'llm_slo_agent_ttft_drift_distance{service="rag"}' not in text, "an empty sample: no series"
    for reason in dr.EVENT_STATS:
        assert v[f'llm_slo_agent_ttft_drift_events_total{{reason="{reason}"}}'] == 2 * stats[reason]


@pytest.mark.timeout(120)
def test_the_agent_logs_a_drift_entry_per_scored_group_and_off_means_nothing_new(tmp_path):
    from llm_slo_ebpf_toolkit_amd.contracts import validator

    a, rows, out = _agent(tmp_path, "on", ttft_drift=True, drift_recent_windows=2, drift_gap_windows=1, drift_baseline_windows=3)
    assert rows and all("drift" in r and "gate" not in r for r in rows)
    assert a.specs[0].ttft_drift == (2, 1, 3) and a.specs[0].drift_crit == 4.0 and a.specs[0].drift_min_shift == 2
    assert all(r["drift"]["state"] in ("calm", "slow", "fast", "warming", "rebased") for r in rows)
    emitted = [json.loads(ln) for ln in out.splitlines() if ln.startswith('{"incident_id"')]
    assert emitted
    for d in emitted:
        assert "drift" not in d
        validator.validate("incident-attribution", d)
    text = a.metrics.registry.exposition()
    assert "llm_slo_agent_ttft_drift_state{" in text and 'llm_slo_agent_ttft_drift_events_total{reason="admitted"}' in text
    b, rows_off, out_off = _agent(tmp_path, "off")
    assert b.specs[0].ttft_drift is None and all("drift" not in r and "gate" not in r for r in rows_off)
    assert "llm_slo_agent_ttft_drift_state{" not in b.metrics.registry.exposition()
    assert "llm_slo_agent_ttft_drift_events_total{" not in b.metrics.registry.exposition()
    # the replay is cut by the wall clock, so two runs need not see the same windows: the shapes are compared
    off = [json.loads(ln) for ln in out_off.splitlines() if ln.startswith('{"incident_id"')]
    assert off and {frozenset(d) for d in off} == {frozenset(d) for d in emitted}, "emitted incidents keep their fields"
    assert {frozenset(r) | {"drift"} for r in rows_off} == {frozenset(r) for r in rows}


# ---- the gate -----------------------------------------------------------------------------------------

CALM, SHIFTED, RATE = 120, 30, 20
SEEDS = tuple(range(12))


def _stream(seed):
    rng = np.random.default_rng(seed)
    return [sc.lognormal_window(rng, RATE, 400.0 * (1.3 if w >= CALM else 1.0)) for w in range(CALM + SHIFTED)]


def test_the_oracle_flags_the_shift_within_R_windows_and_no_decided_calm_step():
    """Per seed: Poisson(20) requests a window, TTFT log-normal(log 400, 0.25) in float32 for 120 calm windows,
    then the median at 520 ms, still under the 800 ms SLO; R = L = 10, B = 60, every threshold at its default."""
    for seed in SEEDS:
        o = dr.DriftOracle(span_cap=256, group_cap=1, recent=10, gap=10, baseline=60)
        st = np.array([int(o.results(o.step_records(w, 1), 1)["state"][0]) for w in _stream(seed)])
        decided = (st[:CALM] & dr.WARMING) == 0
        first = np.nonzero(st[CALM:] & dr.SLOW)[0]
        print(f"seed {seed}: decided calm steps {int(decided.sum())}, slow among them {int((st[:CALM] & dr.SLOW).sum())}, "
              f"first slow {int(first[0]) + 1 if len(first) else None} windows after the change")
        assert int(decided.sum()) >= CALM - 35 and not (st[:CALM] & dr.SLOW).any(), seed
        assert len(first) and int(first[0]) + 1 <= 10, seed


def _decisions(tmp_path, tag, results, **kw):
    """Every window's results through the agent's emission gate (Agent._attributions); the decision log's rows."""
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions

    log = tmp_path / f"gate-{tag}.jsonl"
    o = AgentOptions(engine="cpu", source="replay", gpus=1, window_ms=1000, metrics_bind="", output="stdout", config="",
                     ring_name=f"/mislo-drg-{tag}-{os.getpid()}", min_confidence=0.0, decision_log=str(log), ttft_slo_ms=800.0,
                     ttft_drift=True, **kw)
    a = Agent(o, out_stream=io.StringIO())
    try:
        model, _image, _meta = a._load_model()
        incidents = [a._attributions(1, ["chat"], r, 1_700_000_000_000_000_000 + w * 10 ** 9, model) for w, r in enumerate(results)]
    finally:
        a.close()
    rows = [json.loads(ln) for ln in log.read_text().splitlines()]
    assert len(rows) == len(results) - sum(1 for r in results if r["sli"][0, 0] == 0)
    return rows, incidents


@pytest.mark.timeout(120)
def test_the_emission_gate_widens_with_emit_on_drift_only(tmp_path):
    """The seeded stream through the host engine, every window's results through the agent's gate. The shifted
    phase breaches now and then (about 4 % of a log-normal about 520 ms lies above 800 ms), so some of its windows
    burn on their own; the windows between them do not. ``recovered`` is untouched and holds back a window of at
    least 4 requests a second without a breach whatever opened the gate, so the runs that look for drift-gated
    windows switch that rule off (--emit-recovered-requests 0); the last run keeps it."""
    results, tracked = sc.run_pipeline("cpu", _stream(SEEDS[0]), 1, (10, 10, 60), group_cap=2)
    assert all(set(dr.RESULT_KEYS) <= set(r) for r in results)
    t0 = 1_700_000_000_000_000_000
    shifted = lambda rows: [r for r in rows if r["t_ns"] >= t0 + CALM * 10 ** 9]  # noqa: E731
    calm = lambda rows: [r for r in rows if r["t_ns"] < t0 + CALM * 10 ** 9]  # noqa: E731
    off, inc_off = _decisions(tmp_path, "off", results, emit_recovered_requests=0)
    on, inc_on = _decisions(tmp_path, "on", results, emit_on_drift=True, emit_recovered_requests=0)
    assert all("gate" not in r for r in off) and all(r["why"] != "emitted" or r["gate"] in ("burn", "drift") for r in on)
    slow_quiet = [r for r in shifted(off) if r["drift"]["state"] == "slow" and r["why"] == "no_burn"]
    assert slow_quiet and not any(r["emitted"] for r in slow_quiet), "without the flag a slow service that does not burn is silent"
    by_drift = [r for r in shifted(on) if r.get("gate") == "drift"]
    assert by_drift and all(r["emitted"] and r["why"] == "emitted" and r["drift"]["state"] == "slow" for r in by_drift)
    assert {r["t_ns"] for r in by_drift} == {r["t_ns"] for r in slow_quiet}
    assert not any(r.get("gate") == "drift" for r in calm(on))
    # the burn gate's own decisions are the same with and without the flag
    assert [r["t_ns"] for r in on if r.get("gate") == "burn"] == [r["t_ns"] for r in off if r["emitted"]]
    assert sum(len(x) for x in inc_on) == sum(len(x) for x in inc_off) + len(by_drift)
    quoted = {a.timestamp: a for x in inc_on for a in x}
    for r in by_drift:   # the incident contract is closed: a drift-gated incident quotes the forecast burn it has
        assert quoted[r["t_ns"]].slo_impact.burn_rate == r["burn_forecast"]
        d = r["drift"]   # the baseline is the calm phase's; the recent sample may still mix both phases
        assert 380.0 < d["p50_ms"][0] < 420.0 and d["distance"] > 0 and d["held_windows"] >= 1
        assert d["p50_ms"][1] > d["p50_ms"][0] or d["p90_ms"][1] > d["p90_ms"][0]
    # with the recovered rule at its default a drift-gated window is one it does not hold back
    kept, _ = _decisions(tmp_path, "kept", results, emit_on_drift=True)
    assert all(r["breaches"] > 0 or r["requests"] < 4 for r in kept if r.get("gate") == "drift")
    assert [r["t_ns"] for r in kept if r.get("gate") == "burn"] == [r["t_ns"] for r in _decisions(tmp_path, "plain", results)[0] if r["emitted"]]


# ---- the tracker's host side under the host sanitizers ------------------------------------------------

@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="needs g++")
@pytest.mark.timeout(300)
def test_drift_host_side_under_address_and_ub_sanitizers(tmp_path):
    """ops/csrc/drift_host.h (layout, validate and its messages, ranges, the reduction's packing, crit_q and the
    decision at the edges of 64 bits) needs no device: a stand-alone program over it, built with
    AddressSanitizer + UBSan, run as a child process. It prints the layout of several group counts, which
    must be the Python mirror's."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "llm_slo_ebpf_toolkit_amd", "ops", "csrc")
    exe = tmp_path / "drift_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-Wall", "-Werror", f"-I{csrc}", os.path.join(root, "tests", "native", "drift_host_check.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "drift host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
    got = [tuple(int(x) for x in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("layout ")]
    assert len(got) == 7
    for g, *at in got:
        off = dr.layout(g)
        assert at == [off[k] for k in (*dr.RESULT_FIELDS, "words")]
