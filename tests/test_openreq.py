"""TTFT breaches counted at the deadline (pipeline/openreq.py): a service exports a start record
when a request starts, the agent keeps the open requests and counts, at every window cut, those
whose start + SLO has passed with no first token -- once; the late record that finally arrives is
taken out of the window it lands in. Here: the start record's mapping and export, the rules window
by window on the host implementation, earlier detection and conservation on a faulted stream, and
the window pipeline's pass-through and defaults. tests/test_openreq_gpu.py holds the device table
against this implementation."""

import os

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.collector import otlp
from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.signals.metadata import Interner
from tests import openreq_scenarios as sc
from tests.openreq_scenarios import MS, T0, cut_of, span
from tests.test_first_token import RES, _early, _final, _json

START = R.SPAN_START | R.SPAN_NO_SLI


# ---- the start record: mapping and export ------------------------------------------------------

def _start(tid, t=T0):
    return (tid, "00000000000000c1", "00000000000000a1", t, t, {"llm.slo.request_start": True})


def test_span_mapper_maps_a_start_span_to_a_start_record():
    assert R.SPAN_START == 8 and R.SPAN_START not in (R.SPAN_LATE, R.SPAN_NO_SLI, R.SPAN_FIRST_TOKEN)
    m = otlp.SpanMapper(otlp.GroupTable(4), Interner().id)
    a, b = f"{1:032x}", f"{2:032x}"
    d = otlp.parse_json(_json([_start(a)]))
    assert m.is_request_span(d[0][1])
    r = m.records(d)
    assert len(r) == 1 and int(r["flags"][0]) == START and np.isnan(r["ttft_ms"][0])
    assert int(r["ts_ns"][0]) == T0 and int(r["trace_h"][0]) == otlp.trace_hash(a)
    assert int(r["pod_id"][0]) != 0 and int(r["pid"][0]) == RES["process.pid"] and int(r["group_id"][0]) == 0
    assert not m._early and not m._final  # the pairing tables are untouched
    # the same trace's first-token record and request span pair exactly as without the start
    r1 = m.records(otlp.parse_json(_json([_early(a, 90.0)])))
    assert int(r1["flags"][0]) == R.SPAN_FIRST_TOKEN
    r2 = m.records(otlp.parse_json(_json(_final(a, 91.0, retr=150.0))))
    assert int(r2["flags"][0]) == R.SPAN_NO_SLI and r2["retr_ms"][0] == np.float32(150.0)
    # a start between the two records of a pair changes nothing either
    m.records(otlp.parse_json(_json([_early(b, 50.0)])))
    early, final = dict(m._early), dict(m._final)
    rs = m.records(otlp.parse_json(_json([_start(b)])))
    assert int(rs["flags"][0]) == START and dict(m._early) == early and dict(m._final) == final
    assert int(m.records(otlp.parse_json(_json(_final(b, 51.0))))["flags"][0]) == R.SPAN_NO_SLI
    # a start record is never flagged late, and a span that carries a TTFT is not a start
    m.slo_ms, m.late_before_ns = 10.0, T0 + 50_000_000
    assert int(m.records(otlp.parse_json(_json([_start(f"{3:032x}")])))["flags"][0]) == START
    both = (f"{4:032x}", "00000000000000d1", "00000000000000a1", T0, T0,
            {"llm.slo.request_start": True, "llm.slo.ttft_ms": 5.0})
    assert int(m.records(otlp.parse_json(_json([both])))["flags"][0]) & R.SPAN_START == 0
    # a child span without the attribute (or with it false) is still no request span
    child = (f"{5:032x}", "00000000000000e1", "00000000000000a1", T0, T0, {"llm.slo.request_start": False})
    assert len(m.records(otlp.parse_json(_json([child])))) == 0


def test_rag_service_exports_the_start_record_first():
    from llm_slo_ebpf_toolkit_amd.demo.rag_service import RagService, StubBackend
    from llm_slo_ebpf_toolkit_amd.runtime import load

    rt = load()
    ring = rt.HostRing(64, 64)
    m = otlp.SpanMapper(otlp.GroupTable(4), Interner().id)
    rx = otlp.OtlpSpanReceiver("127.0.0.1:0", m, ring.push).start()
    try:
        svc = RagService(StubBackend(), otlp_endpoint=rx.endpoint, resource={"k8s.pod.uid": RES["k8s.pod.uid"]},
                         export_start=True)
        outs = [svc.chat({"prompt": f"start record {i}", "profile": "chat_short", "max_tokens": 3}) for i in range(3)]
        svc.spans.flush()
    finally:
        rx.stop()
    buf = ring.records_view()[: ring.size * 64].view(R.SPAN)
    assert ring.size == 9
    for o in outs:
        mine = buf[buf["trace_h"] == np.uint64(otlp.trace_hash(o["trace_id"]))]
        assert [int(f) for f in mine["flags"]] == [START, R.SPAN_FIRST_TOKEN, R.SPAN_NO_SLI]  # the start comes first
        assert np.isnan(mine["ttft_ms"][0]) and float(mine["retr_ms"][0]) == 0.0
        assert mine["ts_ns"][0] == mine["ts_ns"][1] == mine["ts_ns"][2]  # the request's start on all three
        assert mine["pod_id"][0] == mine["pod_id"][1] and mine["group_id"][0] == mine["group_id"][1]
        assert float(mine["retr_ms"][1]) > 0  # the retrieval breakdown still rides on the first-token record


# ---- the rules, window by window -----------------------------------------------------------------

def _oracle(**kw):
    from llm_slo_ebpf_toolkit_amd.pipeline.openreq import OpenRequestOracle

    kw.setdefault("cap", 64)
    kw.setdefault("slo_ms", 800.0)
    kw.setdefault("reorder_ms", 2000.0)
    return OpenRequestOracle(**kw)


def S(h, g, start_ms):
    return span(T0 + int(start_ms * MS), h, g, np.nan, START)


def F(h, g, start_ms, ttft_ms, flags=R.SPAN_FIRST_TOKEN):
    return span(T0 + int(start_ms * MS), h, g, ttft_ms, flags)


def _step(t, w, recs, G=3):
    from llm_slo_ebpf_toolkit_amd.pipeline.openreq import stats_dict

    spans = np.concatenate(recs) if recs else np.zeros(0, R.SPAN)
    i = t.step_records(spans, cut_of(w), cut_of(w - 1) if w else 0, G)
    r = t.results(i, G)
    return r["dl"].astype(int), r["dup"].astype(int), stats_dict(r["stats"])


def _rows(t):
    from llm_slo_ebpf_toolkit_amd.pipeline import openreq as O

    k, tt, g, s = t.entries()
    names = {O.OPEN: "open", O.COUNTED: "counted", O.RESOLVED: "resolved"}
    return {int(a): (int(b) - T0, int(c), names[int(d)]) for a, b, c, d in zip(k, tt, g, s)}


@pytest.mark.parametrize("order", ["start_first", "first_token_first"])
def test_start_and_first_token_in_one_window(order):
    t = _oracle()
    recs = [S(11, 0, 100), F(11, 0, 100, 90.0)]
    dl, dup, st = _step(t, 0, recs if order == "start_first" else recs[::-1])
    assert not dl.any() and not dup.any() and _rows(t) == {}
    assert (st["starts"], st["resolves"], st["live_open"], st["live_resolved"]) == (1, 1, 0, 0)
    dl, dup, st = _step(t, 1, [F(11, 0, 100, 90.0, R.SPAN_NO_SLI)])  # the request span: skipped entirely
    assert st["resolves"] == 0 and _rows(t) == {}


def test_first_token_a_window_before_its_start_and_marker_expiry():
    t = _oracle()
    dl, dup, st = _step(t, 0, [F(12, 1, 900, 50.0)])
    assert _rows(t) == {12: (cut_of(0) - T0, 1, "resolved")} and st["live_resolved"] == 1
    dl, dup, st = _step(t, 1, [S(12, 1, 900)])  # the marker drops the start: it never opens, never counts
    assert st["start_after_sli"] == 1 and st["dup_start"] == 0 and _rows(t) == {12: (cut_of(0) - T0, 1, "resolved")}
    dl, dup, st = _step(t, 2, [])  # born at cut 0, reorder 2 s: gone at cut 2
    assert _rows(t) == {} and st["live_resolved"] == 0 and not dl.any()
    for w in (3, 4):
        assert not _step(t, w, [])[0].any()


def test_duplicate_start():
    t = _oracle()
    dl, dup, st = _step(t, 0, [S(13, 2, 700), S(13, 2, 700)])
    assert st["dup_start"] == 1 and _rows(t) == {13: (700 * MS, 2, "open")}
    dl, dup, st = _step(t, 1, [S(13, 2, 700)])  # counted at this cut (deadline 1.5 s), once
    assert st["dup_start"] == 1 and dl.tolist() == [[0, 0], [0, 0], [1, 0]] and _rows(t)[13][2] == "counted"
    dl, dup, st = _step(t, 2, [S(13, 2, 700)])  # a start of a counted request is a duplicate too
    assert st["dup_start"] == 1 and not dl.any()


def test_deadline_in_this_window_or_before_the_previous_cut():
    t = _oracle()
    dl, dup, st = _step(t, 0, [S(21, 0, 100), S(22, 1, 500)])
    assert dl.tolist() == [[1, 0], [0, 0], [0, 0]]  # 21: deadline 0.9 s < cut 0; 22: 1.3 s, still open
    assert _rows(t) == {21: (100 * MS, 0, "counted"), 22: (500 * MS, 1, "open")}
    dl, dup, st = _step(t, 1, [])
    assert dl.tolist() == [[0, 0], [1, 0], [0, 0]]  # 22's deadline lies in window 1
    # a start record exported two windows late (a starved service): its deadline passed before cut 1
    dl, dup, st = _step(t, 2, [S(23, 2, 150)])
    assert dl.tolist() == [[0, 0], [0, 0], [0, 1]] and _rows(t)[23] == (150 * MS, 2, "counted")
    # a deadline exactly on the cut has not passed; one exactly on the previous cut is this window's
    t2 = _oracle()
    dl, dup, st = _step(t2, 0, [S(24, 0, 200)])
    assert not dl.any()
    assert _step(t2, 1, [])[0].tolist() == [[1, 0], [0, 0], [0, 0]]


def test_counted_request_reports_late_breaching_or_within_the_slo():
    from llm_slo_ebpf_toolkit_amd.pipeline.openreq import correct_results

    t = _oracle()
    _step(t, 0, [S(31, 0, 100), S(32, 1, 100), S(33, 2, 100), S(34, 2, 120)])
    assert [r[2] for r in _rows(t).values()] == ["counted"] * 4
    recs = [F(31, 0, 100, 1500.0, R.SPAN_FIRST_TOKEN | R.SPAN_LATE),  # the receiver flagged it late
            F(32, 1, 100, 1500.0),                                    # a breach, not flagged (pushed directly)
            F(33, 2, 100, 700.0, R.SPAN_FIRST_TOKEN | R.SPAN_LATE),   # within the SLO after all
            F(34, 2, 120, 800.0)]                                     # exactly the SLO: no breach
    dl, dup, st = _step(t, 1, recs)
    assert dup.tolist() == [[0, 0, 1], [1, 1, 0], [2, 0, 0]] and st["false_deadline"] == 2 and _rows(t) == {}
    # the corrected counts take the engine's count of these records back out of window 1
    sli, late = sc.engine_counts(np.concatenate(recs), 3)
    assert sli.tolist() == [[0, 0], [1, 1], [2, 0]] and late[:, 0].tolist() == [1, 0, 0]
    c = correct_results({"sli": sli, "late": late}, {"dl": dl, "dup": dup})
    assert not c["sli"].any() and not c["late"].any()
    assert (c["sli_raw"] == sli).all() and (c["late_raw"] == late).all()
    assert (c["deadline"] == dl).all() and (c["deadline_dup"] == dup).all()
    assert c["sli"].dtype == sli.dtype and c["late"].dtype == late.dtype


def test_ttl_expiry():
    t = _oracle(ttl_ms=3000.0)
    assert _step(t, 0, [S(41, 0, 100)])[0][0, 0] == 1
    for w in (1, 2):
        dl, dup, st = _step(t, w, [])
        assert st["expired"] == 0 and st["live_counted"] == 1 and not dl.any()
    dl, dup, st = _step(t, 3, [])  # cut 3 - start = 3.9 s >= 3 s
    assert st["expired"] == 1 and st["live_counted"] == 0 and _rows(t) == {}
    # its record after that finds nothing: a marker, no correction
    dl, dup, st = _step(t, 4, [F(41, 0, 100, 4500.0, R.SPAN_FIRST_TOKEN | R.SPAN_LATE)])
    assert not dup.any() and st["live_resolved"] == 1


def test_records_outside_the_groups_or_without_a_trace_are_ignored():
    t = _oracle()
    dl, dup, st = _step(t, 0, [S(51, 3, 100), S(0, 0, 100), F(0, 0, 100, 2000.0), S(52, 7, 100)], G=3)
    assert st["starts"] == 0 and st["resolves"] == 0 and _rows(t) == {} and not dl.any()
    # a counted request whose record names a group outside the window's: removed, nothing taken back
    assert _step(t, 1, [S(53, 1, 1100)], G=3)[0][1, 0] == 1  # deadline 1.9 s < cut 1
    assert not _step(t, 2, [], G=3)[0].any()
    dl, dup, st = _step(t, 3, [F(53, 5, 1100, 2500.0)], G=3)
    assert not dup.any() and _rows(t) == {}


def test_oracle_checks_its_arguments_and_keeps_the_last_steps():
    t = _oracle(n_buffers=2)
    with pytest.raises(ValueError):
        t.step_records(np.zeros(0, R.SPAN), 0, 0, 3)
    with pytest.raises(ValueError):
        t.step_records(np.zeros(0, R.SPAN), cut_of(0), cut_of(1), 3)
    with pytest.raises(ValueError):
        t.step_records(np.zeros(0, R.SPAN), cut_of(0), 0, 65)
    for w in range(3):
        _step(t, w, [])
    t.results(2, 3), t.results(1, 3)
    with pytest.raises(KeyError):
        t.results(0, 3)


# ---- earlier detection and conservation ------------------------------------------------------------

def test_deadline_counting_detects_the_fault_earlier_and_counts_every_request_once():
    from llm_slo_ebpf_toolkit_amd.pipeline.openreq import correct_results

    st = sc.stream(seed=5, n_groups=3, per_window=30, n_windows=14, fault_window=5, fault_group=1)
    assert st.n_breaching > 20
    t = _oracle(cap=1 << 12)
    raw, cor = [], []

    def each(w, res):
        sli, late = sc.engine_counts(st.windows[w], st.n_groups)
        raw.append((sli, late))
        cor.append(correct_results({"sli": sli, "late": late}, res))

    sc.run(t, st, each)
    fw, fg = st.fault_window, st.fault_group
    first_cor = min(w for w, c in enumerate(cor) if c["sli"][:, 1].any() or c["late"][:, 0].any())
    first_raw = min(w for w, (s, la) in enumerate(raw) if s[:, 1].any() or la[:, 0].any())
    assert first_cor <= fw + 1, (first_cor, fw)
    assert first_raw >= fw + 3, (first_raw, fw)
    assert cor[first_cor]["sli"][fg, 1] > 0 and not np.delete(cor[first_cor]["sli"][:, 1], fg).any()
    # every request has reported: each counted once, each breach once (in its window, or late)
    assert t.entries()[0].size == 0
    assert sum(int(c["sli"][:, 0].sum()) for c in cor) == st.n_requests
    assert sum(int(c["sli"][:, 1].sum()) + int(c["late"][:, 0].sum()) for c in cor) == st.n_breaching
    # the raw counts conserve too, only later
    assert sum(int(s[:, 1].sum()) + int(la[:, 0].sum()) for s, la in raw) == st.n_breaching
    # no false deadline, no duplicate, nothing dropped on this stream
    tot = np.sum([r["stats"] for r in sc.run(_oracle(cap=1 << 12), st)], axis=0)
    assert tot[:5].tolist() == [0, 0, 0, 0, 0]


# ---- the window pipeline ---------------------------------------------------------------------------

RESULT_KEYS = {"post", "conf", "feat", "pred", "evbits", "sli", "app", "late"}


def _pipe_run(wins, tag, with_starts):
    from llm_slo_ebpf_toolkit_amd.models.bayes import NaiveBayes
    from llm_slo_ebpf_toolkit_amd.pipeline.window import RingWindowSource, WindowPipeline, build_replay_images
    from tests.test_native_engine import feed, pod_meta, rings

    for w in wins:
        sp = w.spans0
        if with_starts:  # every 2nd request also says "started"
            s = sp[::2].copy()
            s["flags"], s["ttft_ms"], s["retr_ms"], s["conn_h"] = START, np.nan, 0.0, 0
            sp = np.concatenate([s, sp])
            sp = sp[np.argsort(sp["ts_ns"], kind="stable")]
        w.spans = sp
    imgs = build_replay_images(wins, user_rec=24)
    pipe = WindowPipeline(16384, 1024, 8, model="bayes_gpu", learn=False, user_cap=4096, engine="cpu")
    assert pipe.tracker is None
    pipe.set_model(NaiveBayes.gpu())
    rb, user, spans = rings(tag, 24)
    src = RingWindowSource(pipe, rb, user, spans)
    pipe.eng.set_pods(*pod_meta(wins[0].gen))
    out = []
    for w, img in zip(wins, imgs):
        k = src.stage(feed(img, rb, user, spans), w.n_groups, img.labels)["k"]
        out.append((np.array(pipe.packet(k)["dbg"][:5], copy=True), pipe.results(k, w.n_groups)))
    src.drain()
    pipe.close()
    return out


def test_start_records_join_and_never_count_and_the_defaults_are_unchanged():
    from tests.test_native_engine import windows

    wins, gen = windows(n_win=2, seed=7)
    for w in wins:
        w.spans0, w.gen = w.spans.copy(), gen
    plain = _pipe_run(wins, f"or{os.getpid()}p", False)
    started = _pipe_run(wins, f"or{os.getpid()}s", True)
    for j, ((d0, r0), (d1, r1)) in enumerate(zip(plain, started)):
        assert set(r0) == RESULT_KEYS and set(r1) == RESULT_KEYS  # open_requests=0: today's dict
        assert d1[0] > d0[0], f"window {j}: the start records join ({d0[0]} -> {d1[0]})"
        for key in ("sli", "late", "app"):
            np.testing.assert_array_equal(r0[key], r1[key], err_msg=f"window {j} {key}")
        assert r0["sli"][:, 0].sum() == len(wins[j].spans0)


def test_pipeline_with_the_tracker_on_the_host_engine():
    """engine="cpu" + open_requests: the oracle steps with the rings' span ranges and the cuts'
    times; results() carries the corrected and the raw counts; a cut without a time is skipped."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import WindowPipeline

    st = sc.stream(seed=5, n_groups=3, per_window=30, n_windows=14, fault_window=5, fault_group=1)
    res, stats, pipe_stats = sc.run_pipeline("cpu", st, f"orc{os.getpid()}")
    ref = _oracle(cap=1 << 12)
    want = sc.run(ref, st)
    for w, (r, tr) in enumerate(zip(res, want)):
        assert set(r) == RESULT_KEYS | {"sli_raw", "late_raw", "deadline", "deadline_dup"}
        sli, late = sc.engine_counts(st.windows[w], st.n_groups)
        np.testing.assert_array_equal(r["sli_raw"], sli, err_msg=f"window {w}")
        np.testing.assert_array_equal(r["late_raw"], late, err_msg=f"window {w}")
        np.testing.assert_array_equal(r["deadline"], tr["dl"], err_msg=f"window {w}")
        np.testing.assert_array_equal(r["deadline_dup"], tr["dup"], err_msg=f"window {w}")
        np.testing.assert_array_equal(stats[w], tr["stats"], err_msg=f"window {w}")
    assert sum(int(r["sli"][:, 0].sum()) for r in res) == st.n_requests
    assert sum(int(r["sli"][:, 1].sum()) + int(r["late"][:, 0].sum()) for r in res) == st.n_breaching
    assert pipe_stats["skipped"] == 1  # the trailing cut without a time
    # one GPU only: a communicator or a shard of a node's stream is refused
    with pytest.raises(ValueError, match="one GPU"):
        WindowPipeline(1024, 64, 4, engine="cpu", shard=(0, 2), open_requests=64)


def test_agent_flags_and_the_one_gpu_rule():
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions
    from llm_slo_ebpf_toolkit_amd.cli.agent import parse

    o, _ = parse(["--engine", "cpu", "--deadline-breach", "--open-requests-cap", "4096"])
    assert o.deadline_breach and o.open_requests_cap == 4096
    assert not parse([])[0].deadline_breach and AgentOptions().open_requests_cap == 1 << 20
    a = Agent(AgentOptions(engine="cpu", source="replay", gpus=2, deadline_breach=True, config="", output="stdout",
                           metrics_bind="", ring_name=f"/mislo-or2-{os.getpid()}"))
    try:
        with pytest.raises(ValueError, match="one GPU"):
            a.run_windows(max_windows=1)
    finally:
        a.close()


@pytest.mark.timeout(120)
def test_agent_runs_with_deadline_breach_and_exports_the_table(tmp_path):
    import io
    import json

    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions
    from llm_slo_ebpf_toolkit_amd.export.prometheus import parse_exposition

    log = tmp_path / "decisions.jsonl"
    o = AgentOptions(engine="cpu", source="replay", gpus=1, window_events=2048, window_spans=128, window_groups=8,
                     window_ms=300, metrics_bind="", output="stdout", ring_name=f"/mislo-or1-{os.getpid()}",
                     config="", min_confidence=0.0, scenario="full", disable_overhead_guard=True,
                     deadline_breach=True, open_requests_cap=1 << 12, decision_log=str(log))
    a = Agent(o, out_stream=io.StringIO())
    try:
        assert a.run_windows(max_windows=4) == 0
    finally:
        a.close()
    assert {"sli_raw", "late_raw", "deadline", "deadline_dup"} <= set(a.last_results)
    # the replay's services export no start records: nothing opens, nothing is corrected
    np.testing.assert_array_equal(a.last_results["sli"], a.last_results["sli_raw"])
    m = parse_exposition(a.metrics.registry.exposition())
    assert 'llm_slo_agent_open_requests{state="resolved"}' in m
    assert m['llm_slo_agent_open_requests{state="open"}'] == 0
    assert m['llm_slo_agent_open_request_events_total{reason="dropped_full"}'] == 0
    rows = [json.loads(ln) for ln in log.read_text().splitlines()]
    assert rows and all(r["deadline"] == [0, 0] for r in rows)


def test_open_request_metrics():
    from llm_slo_ebpf_toolkit_amd.agent.metrics import AgentMetrics
    from llm_slo_ebpf_toolkit_amd.export.prometheus import parse_exposition

    m = AgentMetrics("probe", "auto", [], [])
    m.observe_open_requests(np.array([[2, 1], [0, 0]]), {"live_open": 5, "live_counted": 2, "live_resolved": 1,
                                                         "dup_start": 3, "false_deadline": 1}, ["rag", "tp"])
    v = parse_exposition(m.registry.exposition())
    assert v['llm_slo_agent_deadline_breaches_total{service="rag"}'] == 3
    assert v['llm_slo_agent_open_requests{state="counted"}'] == 2
    assert v['llm_slo_agent_open_request_events_total{reason="dup_start"}'] == 3
    assert v['llm_slo_agent_open_request_events_total{reason="expired"}'] == 0


# ---- the tracker's host side under the host sanitizers ------------------------------------------------

@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="needs g++")
@pytest.mark.timeout(300)
def test_tracker_host_side_under_address_and_ub_sanitizers(tmp_path):
    """ops/csrc/openreq_host.h (argument checks, result layout, result-slot bookkeeping) needs no
    device: a stand-alone program over it, built with AddressSanitizer + UBSan."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "llm_slo_ebpf_toolkit_amd", "ops", "csrc")
    exe = tmp_path / "openreq_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-Wall", "-Werror", f"-I{csrc}", os.path.join(root, "tests", "native", "openreq_host_check.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "openreq host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
