"""The decode SLI's rules on the host (pipeline/decodesli.py): the bucket rule against ``lower`` over the whole
range, the numpy oracle against a per-record loop on every named case (tests/decodesli_scenarios.py CASES),
every refusal, the TPOT field of a span's flags and the receiver that fills it (collector/otlp.py
``decode_sli``), the claim that every other reader tests the flag bits by mask (the five other oracles on a
window with and without a TPOT packed in), the host engine's result keys, the agent's flags, decision-log
entry and series, and the tracker's host side (ops/csrc/decodesli_host.h) under the host sanitizers. The
device tracker against the oracle: tests/test_decodesli_gpu.py."""

import io
import json
import os

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.collector import otlp
from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.contracts import semconv
from llm_slo_ebpf_toolkit_amd.pipeline import decodesli as ds
from llm_slo_ebpf_toolkit_amd.signals.metadata import Interner
from tests import decodesli_scenarios as sc
from tests.test_first_token import T0, _early, _json


def test_the_bucket_rule_against_lower_over_the_whole_range():
    u = np.arange(1, R.SPAN_TPOT_MAX + 1)
    b = ds.bucket_of(u)
    assert int(b.min()) == 1 and int(b.max()) == ds.K - 1 == 335 and (np.diff(b) >= 0).all() and (np.diff(b) <= 1).all()
    assert (ds.lower(b) <= u).all() and (u < ds.lower(b + 1)).all()
    assert int(ds.bucket_of(100_000)) == 216 and int(ds.lower(216)) == 98_304 and int(ds.lower(217)) == 102_400
    assert all(int(ds.bucket_of(x)) == sc.brute_bucket(x) for x in sc.EDGE_US)
    rep = ds.representative()
    assert rep.shape == (ds.K,) and (rep[:16] == np.arange(16)).all()
    lo = ds.lower(np.arange(16, ds.K)).astype(np.float64)
    assert (np.abs(rep[16:] - lo) <= lo / 32).all() and (np.abs(ds.lower(np.arange(17, ds.K + 1)) - 1 - rep[16:]) <= lo / 32).all()
    assert ds.tpot_slo_us(100.0) == 100_000 and ds.tpot_slo_us(1e-9) == 1 and ds.tpot_slo_us(1e9) == R.SPAN_TPOT_MAX


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_oracle_equals_the_per_record_loop_after_every_step(name):
    c = sc.case(name)
    o, brute = ds.DecodeSliOracle(**c.cfg), sc.Brute(**c.cfg)
    C = c.cfg["group_cap"]
    seen = []
    for w, (recs, G) in enumerate(c.steps):
        want = brute.step(recs, G)
        got = o.results(o.step_records(recs, G), C)
        sc.same_results(got, want, f"{name} step {w}")
        sc.same_resident(o.resident(), brute.resident(), f"{name} step {w}", pos=False)
        assert o.resident()["pos"] == (w + 1) % c.cfg["windows"]
        for f in ds.RESULT_FIELDS[:-1]:
            np.testing.assert_array_equal(o.results(w, G)[f], want[f][:G], err_msg=f"{name} step {w} first G rows of {f}")
        blk, off = o.block(w), ds.layout(C)
        assert blk.dtype == np.uint32 and len(blk) == off["words"] and all(v % 4 == 0 for v in off.values())
        np.testing.assert_array_equal(blk[off["sum_us"]:off["sum_us"] + 2 * C].view(np.uint64), want["sum_us"])
        np.testing.assert_array_equal(blk[off["q_roll"]:off["q_roll"] + 4 * C].reshape(C, 4), want["q_roll"])
        seen.append(got)
    if c.check is not None:
        c.check(seen)


def test_every_configuration_check_and_every_refused_step():
    for kw, msg in ((dict(windows=0), "windows"), (dict(windows=4097), "windows"), (dict(group_cap=0), "group_cap"),
                    (dict(group_cap=65537), "group_cap"), (dict(span_cap=0), "span_cap"), (dict(n_buffers=0), "n_buffers"),
                    (dict(n_buffers=65), "n_buffers"), (dict(slo_ms=-1.0), "slo_ms"), (dict(slo_ms=float("nan")), "slo_ms"),
                    (dict(slo_ms=float("inf")), "slo_ms"), (dict(tpot_slo_ms=0.0), "tpot_slo_ms"),
                    (dict(tpot_slo_ms=float("nan")), "tpot_slo_ms"), (dict(tpot_slo_ms=float("inf")), "tpot_slo_ms"),
                    (dict(span_cap=1 << 21, windows=2048), "below 2"), (dict(group_cap=65536, windows=4096), "2 GiB")):
        with pytest.raises(ValueError, match=msg):
            ds.DecodeSliOracle(**kw)
    ds.DecodeSliOracle(windows=1, group_cap=1, span_cap=1, n_buffers=1, slo_ms=0.0, tpot_slo_ms=1e-9).close()
    rng = np.random.default_rng(5)
    recs = np.ascontiguousarray(sc.mixed_window(rng, 50, 3))
    o = ds.DecodeSliOracle(**sc._cfg(span_cap=len(recs)))
    o.step_records(recs, 3)
    before = {k: np.array(v, copy=True) for k, v in o.resident().items()}
    a = recs.ctypes.data
    for bad in (lambda: o.step([(a, 63)], 3), lambda: o.step([(0, 64)], 3), lambda: o.step_records(recs, 4),
                lambda: o.step_records(recs, -1), lambda: o.step_records(np.concatenate([recs, recs[:1]]), 3)):
        with pytest.raises(ValueError, match="decode sli step"):
            bad()
    sc.same_resident(o.resident(), before, "a refused step changes nothing")
    assert o.step([(a, 64 * 10), (a + 640, 0), (a + 640, 64 * 5)], 3) == 1
    brute = sc.Brute(**sc._cfg())
    brute.step(recs, 3)
    sc.same_results(o.results(1, 3), brute.step(recs[:15], 3), "the step after the refused ones")
    with pytest.raises(IndexError):
        o.results(5, 3)


# ---- the value on the wire ----------------------------------------------------------------------------

def test_the_tpot_field_of_the_flags_word():
    assert (R.SPAN_TPOT_SHIFT, R.SPAN_TPOT_MAX) == (8, (1 << 24) - 1)
    for us in (0, 1, 100_000, R.SPAN_TPOT_MAX):
        for low in (0, R.SPAN_LATE, R.SPAN_NO_SLI | R.SPAN_LATE, 0xFF):
            assert R.span_tpot_us(low | R.pack_tpot_us(us)) == us and (low | R.pack_tpot_us(us)) & 0xFF == low
    arr = np.array([0, 7, R.SPAN_TPOT_MAX], np.int64)
    np.testing.assert_array_equal(R.span_tpot_us(R.pack_tpot_us(arr) | np.uint32(R.SPAN_NO_SLI)), arr)
    for bad in (-1, R.SPAN_TPOT_MAX + 1):
        with pytest.raises(ValueError):
            R.pack_tpot_us(bad)
        with pytest.raises(ValueError):
            R.pack_tpot_us(np.array([bad]))
    assert [R.tpot_us_of_ms(x) for x in (100.0, 0.0004, 0.0016, 16777.2144, 16777.215, 1e12)] == \
        [100_000, 1, 2, 16_777_214, R.SPAN_TPOT_MAX, R.SPAN_TPOT_MAX]
    assert [R.tpot_us_of_ms(x) for x in (0.0, -1.0, float("nan"), float("inf"), float("-inf"), "x", None)] == [0] * 7
    assert semconv.ATTR_SLO_TPOT_MS == "llm.slo.tpot_ms"


def _final(tid, ttft, dur_ms=900.0, **attrs):
    return (tid, "00000000000000a1", "", T0, T0 + int(dur_ms * 1e6), {"llm.slo.ttft_ms": ttft, **attrs})


def _start(tid):
    return (tid, "00000000000000c1", "", T0, T0, {"llm.slo.request_start": True})


def _mapper(**kw):
    return otlp.SpanMapper(otlp.GroupTable(4), Interner().id, **kw)


def _tid(i):
    return f"{i:032x}"


def test_the_mapper_off_is_the_mapper_of_today():
    batch = [_start(_tid(1)), _early(_tid(1), 90.0), _final(_tid(1), 91.0, **{"llm.slo.tpot_ms": 40.0}),
             _final(_tid(2), 50.0, **{"llm.slo.tokens_per_sec": 20.0}),
             _final(_tid(3), 50.0, **{"gen_ai.usage.output_tokens": 11})]
    plain, off, on = _mapper(), _mapper(decode_sli=False), _mapper(decode_sli=True)
    for m in (plain, off, on):
        m.slo_ms, m.late_before_ns = 10.0, T0 + 50_000_000  # every record is late as well
    a, b, c = (m.records(otlp.parse_json(_json(batch))) for m in (plain, off, on))
    assert len(a) == 5 and a.tobytes() == b.tobytes()
    assert a["flags"].tolist() == [R.SPAN_START | R.SPAN_NO_SLI, R.SPAN_FIRST_TOKEN | R.SPAN_LATE, R.SPAN_NO_SLI | R.SPAN_LATE,
                                   R.SPAN_LATE, R.SPAN_LATE]
    # on: bits 0-3 unchanged (SPAN_LATE included), every other field byte-equal
    assert (c["flags"] & np.uint32(0xFF)).tolist() == a["flags"].tolist()
    masked = c.copy()
    masked["flags"] &= np.uint32(0xFF)
    assert masked.tobytes() == a.tobytes()
    # start and first-token records carry none; the request spans one each: tpot_ms, 1000 / rate, (latency - ttft) / (n - 1)
    assert R.span_tpot_us(c["flags"]).tolist() == [0, 0, 40_000, 50_000, 85_000]
    # and through the tracker's rules: three finished requests, all within both SLOs; without the switch, none has a TPOT
    for batch_recs, want in ((c, {"observed": 3, "invalid": 0, "out_of_group": 0, "no_decode": 0}),
                             (a, {"observed": 0, "invalid": 0, "out_of_group": 0, "no_decode": 3})):
        o = ds.DecodeSliOracle(**sc._cfg(group_cap=4))
        r = o.results(o.step_records(batch_recs, 4), 4)
        assert ds.stats_dict(r["stats"]) == want and r["cells"][0].tolist() == [want["observed"], 0, 0, 0]
        assert int(r["sum_us"][0]) == (175_000 if want["observed"] else 0)


def test_the_mapper_s_three_sources_their_precedence_and_the_clamps():
    m = _mapper(decode_sli=True)

    def us(i, ttft=100.0, dur_ms=900.0, **attrs):
        r = m.records(otlp.parse_json(_json([_final(_tid(1000 + i), ttft, dur_ms, **attrs)])))
        assert len(r) == 1 and int(r["flags"][0]) & 0xFF == 0
        return R.span_tpot_us(int(r["flags"][0]))

    tp, rate, toks = "llm.slo.tpot_ms", "llm.slo.tokens_per_sec", "gen_ai.usage.output_tokens"
    assert us(0) == 0, "no source: no decode SLI"
    assert us(1, **{tp: 12.3456}) == 12_346 and us(2, **{rate: 8.0}) == 125_000 and us(3, **{toks: 5}) == 200_000
    assert us(4, **{tp: 10.0, rate: 8.0, toks: 5}) == 10_000, "tpot_ms first"
    assert us(5, **{rate: 8.0, toks: 5}) == 125_000, "then the rate"
    assert us(6, **{tp: float("nan"), rate: 8.0}) == 0, "a source that applies decides, even when it gives nothing"
    assert us(7, **{rate: 0.0, toks: 5}) == 0 and us(8, **{rate: -3.0}) == 0 and us(9, **{rate: float("nan")}) == 0
    assert us(10, **{tp: 0.0}) == 0 and us(11, **{tp: -1.0}) == 0 and us(12, **{tp: float("inf")}) == 0
    assert us(13, **{tp: 0.0001}) == 1 and us(14, **{tp: 1e7}) == R.SPAN_TPOT_MAX, "both clamps"
    assert us(15, **{rate: 1e9}) == 1 and us(16, **{rate: 1e-6}) == R.SPAN_TPOT_MAX
    assert us(17, **{toks: 1}) == 0 and us(18, **{toks: 2}) == 800_000, "n >= 2"
    assert us(19, ttft=950.0, dur_ms=900.0, **{toks: 3}) == 0, "latency below the TTFT: nothing"
    assert us(20, **{tp: 100.0}) == ds.tpot_slo_us(100.0)
    # a request span whose SLI a first-token record counted already carries its TPOT all the same
    m.records(otlp.parse_json(_json([_early(_tid(77), 90.0)])))
    r = m.records(otlp.parse_json(_json([_final(_tid(77), 91.0, **{tp: 33.0})])))
    assert int(r["flags"][0]) == R.SPAN_NO_SLI | R.pack_tpot_us(33_000)
    # a first-token record without a trace id gets no flag from the pairing, and no TPOT either
    early = ("", "00000000000000f1", "00000000000000a1", T0, T0 + 90_000_000,
             {"llm.slo.ttft_ms": 90.0, "llm.slo.ttft_early": True, tp: 33.0})
    r = m.records(otlp.parse_json(_json([early])))
    assert len(r) == 1 and int(r["flags"][0]) == 0


def test_the_five_other_oracles_read_the_flag_bits_by_mask():
    from llm_slo_ebpf_toolkit_amd.pipeline.exemplars import EXEMPLAR, ExemplarOracle
    from llm_slo_ebpf_toolkit_amd.pipeline.onset import OnsetOracle
    from llm_slo_ebpf_toolkit_amd.pipeline.openreq import OpenRequestOracle
    from llm_slo_ebpf_toolkit_amd.pipeline.podrank import PodRankOracle
    from llm_slo_ebpf_toolkit_amd.pipeline.slisketch import SliSketchOracle
    from tests.onset_scenarios import BIN, Q0, cut_of, edge_window

    rng = np.random.default_rng(3)
    G, q = 3, Q0 + 50
    plain = edge_window(rng, 200, G, q, 64)
    plain["trace_h"] = np.arange(1, len(plain) + 1, dtype=np.uint64)  # one record a trace: the open requests are ordered
    plain["pod_id"] = rng.integers(1, 9, len(plain))
    packed = plain.copy()
    packed["flags"] |= R.pack_tpot_us(rng.integers(1, R.SPAN_TPOT_MAX + 1, len(plain)))
    assert (packed["flags"] != plain["flags"]).all() and ((packed["flags"] ^ plain["flags"]) & np.uint32(0xFF) == 0).all()
    cut = cut_of(q)
    made = (lambda: OpenRequestOracle(cap=1 << 10, span_cap=1024, group_cap=G, slo_ms=800.0),
            lambda: SliSketchOracle(span_cap=1024, group_cap=G, windows=2),
            lambda: ExemplarOracle(k=3, windows=2, span_cap=1024, group_cap=G),
            lambda: PodRankOracle(k=3, windows=2, pair_cap=64, span_cap=1024, group_cap=G, slo_ms=800.0),
            lambda: OnsetOracle(bins=64, bin_ns=BIN, ref_ppm=250_000, alarm=3, span_cap=1024, group_cap=G, slo_ms=800.0))
    args = ((cut, cut - 160_000_000, G), (G,), (G,), (G,), (cut, G))
    for make, extra in zip(made, args):
        out = []
        for recs in (plain, packed):
            o = make()
            out.append(o.results(o.step_records(recs, *extra), G))
        a, b = out
        assert set(a) == set(b)
        for key in a:
            x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
            if x.dtype == EXEMPLAR:
                # an exemplar row quotes its record's whole flags word, so it carries the TPOT too: the same
                # records are chosen, and the quoted word is the record's
                assert ((x["flags"] ^ y["flags"]) & np.uint32(0xFF) == 0).all()
                assert (y["flags"][y["trace_h"] != 0] >> np.uint32(8) > 0).all()
                y = y.copy()
                y["flags"] = x["flags"]
            assert x.tobytes() == y.tobytes(), (type(o).__name__, key)


# ---- the pipeline -------------------------------------------------------------------------------------

def test_pipeline_on_the_host_engine_carries_the_new_keys_only_when_switched_on():
    from llm_slo_ebpf_toolkit_amd.pipeline.window import WindowPipeline

    rng = np.random.default_rng(41)
    groups = [3, 3, 2, 3]
    wins = [sc.mixed_window(rng, 40, 3) if w != 2 else np.zeros(0, R.SPAN) for w in range(4)]
    off, none = sc.run_pipeline("cpu", wins, groups, 0)
    onr, dec = sc.run_pipeline("cpu", wins, groups, 2)
    ref = ds.DecodeSliOracle(**sc._cfg(group_cap=8, windows=2))
    assert none == []
    for w, (a, b, d) in enumerate(zip(off, onr, dec)):
        assert not set(a) & set(ds.RESULT_KEYS) and set(b) == set(a) | set(ds.RESULT_KEYS)
        for key in a:
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"window {w} {key}")
        want = ref.results(ref.step_records(wins[w], groups[w]), groups[w])
        sc.same_results(d, want, f"window {w}")
        for key, v in ds.result_keys(want).items():
            np.testing.assert_array_equal(b[key], v, err_msg=f"window {w} {key}")
    assert np.isnan(onr[0]["decode_q"]).sum() == 0 and int(onr[2]["decode_cells"].sum()) == 0 and np.isnan(onr[2]["decode_q"]).all()
    with pytest.raises(ValueError, match="one GPU: no communicator, no sharding"):
        WindowPipeline(1024, 64, 4, engine="cpu", shard=(0, 2), decode_sli=2)
    with pytest.raises(ValueError, match="decode sli: tpot_slo_ms"):
        WindowPipeline(1024, 64, 4, engine="cpu", decode_sli=2, tpot_slo_ms=0.0)
    with pytest.raises(ValueError, match="decode sli: windows"):
        WindowPipeline(1024, 64, 4, engine="cpu", decode_sli=5000)
    p = WindowPipeline(1024, 64, 4, engine="cpu")
    try:
        assert p.decode is None
    finally:
        p.close()


# ---- the agent ----------------------------------------------------------------------------------------

def _agent(tmp_path, tag, **kw):
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions

    log = tmp_path / f"decisions-{tag}.jsonl"
    o = AgentOptions(engine="cpu", source="replay", gpus=1, window_events=2048, window_spans=128, window_groups=8,
                     window_ms=300, metrics_bind="", output="stdout", ring_name=f"/mislo-ds-{tag}-{os.getpid()}",
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

    o, _ = parse(["--engine", "cpu", "--decode-sli", "--tpot-slo-ms", "60", "--decode-horizon-windows", "30"])
    assert (o.decode_sli, o.tpot_slo_ms, o.decode_horizon_windows) == (True, 60.0, 30)
    d = parse([])[0]
    assert (d.decode_sli, d.tpot_slo_ms, d.decode_horizon_windows) == (False, 100.0, 0)
    assert AgentOptions().decode_sli is False
    kw = dict(engine="cpu", source="replay", config="", output="stdout", metrics_bind="")
    a = Agent(AgentOptions(ring_name=f"/mislo-ds2-{os.getpid()}", window_ms=2000, ttft_horizon_windows=40, **kw))
    try:
        assert a.decode_horizon() == a.ttft_horizon() == 40  # the sketch's by default
    finally:
        a.close()
    a = Agent(AgentOptions(ring_name=f"/mislo-ds3-{os.getpid()}", window_ms=2000, decode_horizon_windows=7, **kw))
    try:
        assert a.decode_horizon() == 7 and a.ttft_horizon() == 150
    finally:
        a.close()
    a = Agent(AgentOptions(gpus=2, ring_name=f"/mislo-ds4-{os.getpid()}", decode_sli=True, **kw))
    try:
        with pytest.raises(ValueError, match="--decode-sli runs on one GPU"):
            a.run_windows(max_windows=1)
    finally:
        a.close()


def test_the_decision_log_entry_and_the_series_from_a_fabricated_result():
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent
    from llm_slo_ebpf_toolkit_amd.agent.metrics import AgentMetrics
    from llm_slo_ebpf_toolkit_amd.export.prometheus import parse_exposition

    o = ds.DecodeSliOracle(**sc._cfg(group_cap=3, windows=2))
    o.step_records(sc.recs([sc.FAST] * 6 + [sc.SLOW] * 2, [sc.GOOD] * 8, [1] * 8), 3)
    i = o.step_records(sc.recs([sc.FAST, sc.SLOW, sc.FAST, sc.SLOW], [sc.GOOD, sc.GOOD, sc.BAD, sc.BAD], [1, 1, 1, 2]), 3)
    res = ds.result_keys(o.results(i, 3))
    keys = {"requests", "good", "goodput", "ttft_only", "tpot_only", "both", "tpot_ms"}
    e = [Agent._decode_entry(res, g) for g in range(3)]
    assert all(set(x) == keys | {"horizon"} and set(x["horizon"]) == keys for x in e)
    assert all(set(x["tpot_ms"]) == set(x["horizon"]["tpot_ms"]) == {"p50", "p90", "p95", "p99", "mean"} for x in e)
    empty = {"requests": 0, "good": 0, "goodput": None, "ttft_only": 0, "tpot_only": 0, "both": 0,
             "tpot_ms": dict.fromkeys(("p50", "p90", "p95", "p99", "mean"))}
    assert e[0] == {**empty, "horizon": empty}
    assert {k: e[1][k] for k in ("requests", "good", "goodput", "ttft_only", "tpot_only", "both")} == \
        {"requests": 3, "good": 1, "goodput": round(1 / 3, 6), "ttft_only": 1, "tpot_only": 1, "both": 0}
    assert e[1]["tpot_ms"]["mean"] == round((2 * sc.FAST + sc.SLOW) / 3e3, 4)
    rep = ds.representative() * 1e-3
    assert e[1]["tpot_ms"]["p50"] == round(float(rep[sc.brute_bucket(sc.FAST)]), 4)
    assert e[1]["tpot_ms"]["p99"] == round(float(rep[sc.brute_bucket(sc.SLOW)]), 4)
    assert abs(e[1]["tpot_ms"]["p50"] - sc.FAST * 1e-3) <= sc.FAST * 1e-3 / 32
    h = e[1]["horizon"]
    assert (h["requests"], h["good"], h["ttft_only"], h["tpot_only"], h["both"]) == (11, 7, 1, 3, 0) and h["goodput"] == round(7 / 11, 6)
    assert e[2]["both"] == 1 and e[2]["goodput"] == 0.0
    json.dumps(e)
    m = AgentMetrics("probe", "auto", [], [])
    stats = {"observed": 4, "invalid": 1, "out_of_group": 2, "no_decode": 3}
    m.observe_decode(res, stats, ["rag", "chat"])
    m.observe_decode(res, stats, ["rag", "chat"])
    text = m.registry.exposition()
    v = parse_exposition(text)
    assert v['llm_slo_agent_goodput_ratio{service="chat"}'] == pytest.approx(7 / 11)
    assert v['llm_slo_agent_goodput_ratio{service="group-2"}'] == 0
    assert 'llm_slo_agent_goodput_ratio{service="rag"}' not in text, "no request: no series"
    assert v['llm_slo_agent_tpot_ms{service="chat",quantile="0.5"}'] == pytest.approx(float(rep[sc.brute_bucket(sc.FAST)]))
    assert v['llm_slo_agent_tpot_ms{service="chat",quantile="0.99"}'] == pytest.approx(float(rep[sc.brute_bucket(sc.SLOW)]))
    for outcome, n in zip(ds.CELLS, (1, 1, 1, 0)):
        key = f'llm_slo_agent_decode_requests_total{{service="chat",outcome="{outcome}"}}'
        assert (v[key] == 2 * n) if n else (key not in text)
    for reason in ds.EVENT_STATS:
        assert v[f'llm_slo_agent_decode_events_total{{reason="{reason}"}}'] == 2 * stats[reason]


@pytest.mark.timeout(120)
def test_the_agent_logs_a_decode_entry_per_scored_group_and_off_means_nothing_new(tmp_path):
    from llm_slo_ebpf_toolkit_amd.contracts import validator

    a, rows, out = _agent(tmp_path, "on", decode_sli=True, decode_horizon_windows=3)
    assert rows and all("decode" in r for r in rows)
    assert a.specs[0].decode_sli == 3 and a.specs[0].tpot_slo_ms == 100.0
    emitted = [json.loads(ln) for ln in out.splitlines() if ln.startswith('{"incident_id"')]
    assert emitted
    for d in emitted:
        assert "decode" not in d
        validator.validate("incident-attribution", d)
    # the replay's spans carry no TPOT: every finished request is a no_decode event, the entries are empty
    assert 'llm_slo_agent_decode_events_total{reason="no_decode"}' in a.metrics.registry.exposition()
    assert all(r["decode"]["requests"] == 0 and r["decode"]["goodput"] is None for r in rows)
    b, rows_off, out_off = _agent(tmp_path, "off")
    assert b.specs[0].decode_sli == 0 and all("decode" not in r for r in rows_off)
    assert "llm_slo_agent_decode_events_total{" not in b.metrics.registry.exposition()
    # the replay is cut by the wall clock, so two runs need not see the same windows: the shapes are compared
    off = [json.loads(ln) for ln in out_off.splitlines() if ln.startswith('{"incident_id"')]
    assert off and {frozenset(d) for d in off} == {frozenset(d) for d in emitted}, "emitted incidents keep their fields"
    assert {frozenset(r) | {"decode"} for r in rows_off} == {frozenset(r) for r in rows}


# ---- the tracker's host side under the host sanitizers ------------------------------------------------

@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="needs g++")
@pytest.mark.timeout(300)
def test_decodesli_host_side_under_address_and_ub_sanitizers(tmp_path):
    """ops/csrc/decodesli_host.h (bucket and lower rules over the whole range, the SLO's unit, the cell, the LDS
    key, argument checks, layout, ranges) needs no device: a stand-alone program over it, built with
    AddressSanitizer + UBSan, run as a child process. It prints the layout of several group counts, which
    must be the Python mirror's."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "llm_slo_ebpf_toolkit_amd", "ops", "csrc")
    exe = tmp_path / "decodesli_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-Wall", "-Werror", f"-I{csrc}", os.path.join(root, "tests", "native", "decodesli_host_check.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "decodesli host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
    got = [tuple(int(x) for x in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("layout ")]
    assert len(got) == 7
    for g, *at in got:
        off = ds.layout(g)
        assert at == [off[k] for k in ("cells", "cells_roll", "sum_us", "sum_us_roll", "q_win", "q_roll", "stats", "words")]
