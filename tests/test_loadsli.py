"""The load SLI on the host (pipeline/loadsli.py): the oracle against a per-request, per-bin brute force
on every named case and on seeded random runs, with the in-flight invariants; the duration rule on its
boundary bit patterns; every configuration check and refused step; the pipeline on the host engine (the
new keys only when switched on, every other key byte-equal); the agent's flags and refusals, the decision
log entry and the series; and the tracker's host side under the host sanitizers. No GPU."""

import io
import json
import os

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.pipeline import loadsli as ld
from tests import loadsli_scenarios as sc

F32 = np.float32


# ---- the rules ------------------------------------------------------------------------------------------

def test_dur_us_on_the_boundary_bit_patterns():
    v = np.array([x for x, _ in sc.DUR_PATTERNS], F32)
    assert ld.dur_us(v).tolist() == [w for _, w in sc.DUR_PATTERNS] == [0, 0, 999, 1000, 799999, 3333, 86_400_000_000]
    assert ld.dur_us(v).dtype == np.int64
    # the same through a step: one request per pattern, ending in the ring
    q = sc.QH
    for x, want in sc.DUR_PATTERNS[:-1]:
        o = ld.LoadSliOracle(**sc._cfg(64))
        start = (q + 1) * sc.BIN - 1 - want  # ends in the last microsecond of q_hi
        i = o.step_records(sc.reqs([0], [start], [x]), sc.cut_of(q), 1)
        r = o.results(i, 1)
        assert int(r["stats"][0]) == 1 and int(r["rows"]["busy_ring"][0]) == min(want, 63 * sc.BIN + 999), (x, want)


def _brute_run(c, seen_stats=None):
    ref, br = ld.LoadSliOracle(**c.cfg), sc.Brute(**c.cfg)
    res, resid = [], []
    for w, (recs, cut, G) in enumerate(c.steps):
        what = f"{c.name} step {w}"
        if w in c.refused:
            before = ref.resident()
            with pytest.raises(ValueError, match="ring_records_max"):
                ref.step_records(recs, cut, G)
            sc.same_resident(ref.resident(), before, what)
            res.append(None), resid.append(before)
            continue
        i = ref.step_records(recs, cut, G)
        a = ref.results(i, ref.group_cap)
        sc.same_results(a, br.step(recs, cut, G), what)
        now = ref.resident()
        # the invariants from the ring itself: never a negative number in flight, none after q_hi
        starts, ends, active, busy = ld.per_bin(now["counts"], now["idle_us"], now["carry"], now["q_hi"], ref.bin_us)
        after = now["carry"][:, None] + np.cumsum(starts - ends, axis=1)
        assert (after >= 0).all() and (after[:, -1] == 0).all() and (now["carry"] >= 0).all(), what
        assert (busy >= 0).all() and (busy <= active * ref.bin_us).all(), what
        # the block is the rows and the statistics, every array on 16 bytes
        lay, block = ld.layout(ref.group_cap), ref.block(i)
        assert block.dtype == np.uint32 and len(block) == lay["words"] and lay["stats"] * 4 % 16 == 0
        assert block[:lay["stats"]].tobytes() == a["rows"].tobytes() and block[lay["stats"]:][:8].tolist() == a["stats"].tolist()
        sc.same_rows(ref.results(i, G)["rows"], a["rows"][:G], what)
        res.append(a), resid.append(now)
        if seen_stats is not None:
            seen_stats += a["stats"].astype(np.int64)
    if c.check is not None:
        c.check(res, resid)
    return res


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_oracle_equals_the_brute_force_after_every_step_and_the_hand_computed_expectation(name):
    _brute_run(sc.case(name))


def test_seeded_random_runs_against_the_brute_force_reach_every_placement_case():
    seen = np.zeros(ld.N_STATS, np.int64)
    states = set()
    for seed in range(8):
        B, C = (64, 3) if seed % 2 else (128, 2)
        for r in _brute_run(sc._random(f"random seed {seed}", B, C, 100 + seed, 16, 150), seen):
            states.update(r["rows"]["state"].tolist())
    assert (seen > 0).all(), dict(zip(ld.STATS, seen.tolist()))
    assert {ld.WARMING, ld.STEADY} <= states and len(states) >= 4, states


def test_the_named_cases_cover_the_list():
    names = " | ".join(sc.CASE_NAMES)
    for word in ("inside one bin", "over three bins", "bin boundary", "zero duration", "clipped", "too old", "future start",
                 "future end", "no time", "invalid latencies", "out of group", "skipped", "no-sli finishing", "advance by 0",
                 "B or more", "moving back", "late record", "start evicted", "peak tie", "warming until", "steady", "surge",
                 "slowdown", "drop", "arr_up at equality", "arr_up one below", "arr_down at equality", "arr_down one below",
                 "conc_up at equality", "conc_up one below", "min_requests met", "min_requests missed", "min_conc_milli met",
                 "min_conc_milli missed", "precedence", "age counts", "n_groups changing", "going silent", "long statistic",
                 "ring_records_max", "hot one key", "hot more keys", "hot second workgroup", "hot random"):
        assert word in names, word
    for c in sc.cases():
        assert c.cfg["bins"] in (64, 128) and c.cfg["group_cap"] in (3, 4) and c.cfg["span_cap"] in (256, 512), c.name
        assert c.cfg["bin_us"] == 1000 and all(len(recs) <= c.cfg["span_cap"] for recs, _, _ in c.steps), c.name


def test_classification_helpers_and_the_summary():
    assert ld.classify(6000, 8000, 8, 8, 8, 4, 1000, 1500, 4, 500) == (ld.ARR_UP | ld.CONC_UP, ld.SURGE)
    assert ld.classify(6000, 8000, 8, 8, 8, 4, 1000, 1500, 100, 500) == (ld.CONC_UP, ld.SLOWDOWN)
    assert ld.classify(0, 0, 4, 12, 8, 4, 1000, 1500, 4, 500) == (ld.ARR_DOWN, ld.DROP)
    assert ld.classify(0, 0, 4, 12, 8, 4, 1000, 1501, 4, 500) == (0, ld.STEADY)
    assert [ld.age_of(*x) for x in ((1, 0, 0), (1, 1, 1), (3, 1, 9), (0, 0, 7), (4, 4, 7), (2, 2, 2 ** 32 - 1))] == \
        [1, 2, 1, 0, 0, 2 ** 32 - 1]
    assert ld.ranges_of(1000, 987, 64, 2, 4, 8) == {"oldest": 937, "lo": 987, "recent_lo": 995, "recent_hi": 998, "base_lo": 987,
                                                   "base_hi": 994, "base_bins": 8, "warming": False}
    assert ld.ranges_of(1000, 988, 64, 2, 4, 8)["warming"] and ld.ranges_of(1000, 996, 64, 2, 4, 8)["base_bins"] == 0
    row = np.zeros(1, ld.LOAD_ROW)[0]
    row["state"], row["age"], row["peak_q"], row["peak_active"], row["base_bins"] = ld.SLOWDOWN, 3, 1_700_000_000_123, 7, 8
    row["busy_recent"], row["busy_base"], row["arr_recent"], row["arr_base"] = 6000, 8000, 8, 16
    row["done_recent"], row["done_base"] = 6, 0
    assert ld.summary(row, 1000, 4) == {
        "state": "slowdown", "age_windows": 3, "warming": False, "arrivals_per_s": {"recent": 2000.0, "base": 2000.0},
        "concurrency": {"recent": 1.5, "base": 1.0, "peak": 7, "peak_ts_ns": 1_700_000_000_123 * 1_000_000},
        "service_time_ms": {"recent": 1.0, "base": None}}
    e = ld.summary(ld.warming_rows(1)[0], 1000, 4)
    assert e["state"] == "warming" and e["warming"] and e["arrivals_per_s"] == {"recent": None, "base": None}
    assert e["concurrency"] == {"recent": None, "base": None, "peak": 0, "peak_ts_ns": None}
    assert e["service_time_ms"] == {"recent": None, "base": None}
    json.dumps(e)
    assert ld.empty_result(3)["rows"].tobytes() == ld.warming_rows(3).tobytes() and not ld.empty_result(3)["stats"].any()
    assert set(ld.result_keys(ld.empty_result(2))) == set(ld.RESULT_KEYS) == {"load_rows", "load_stats"}


BAD_CONFIGS = [dict(bins=32), dict(bins=16384), dict(bins=96), dict(bin_us=999), dict(bin_us=60_000_001),
               dict(settle_bins=-1), dict(recent_bins=0), dict(min_base_bins=0), dict(settle_bins=935),
               dict(bins=64, settle_bins=2, recent_bins=4, min_base_bins=59), dict(factor_milli=1000), dict(factor_milli=64001),
               dict(min_requests=0), dict(min_requests=1 << 31), dict(min_conc_milli=0), dict(min_conc_milli=1_000_000_001),
               dict(group_cap=0), dict(group_cap=65537), dict(span_cap=0), dict(n_buffers=0), dict(n_buffers=65),
               dict(ring_records_max=0), dict(ring_records_max=17_592_187), dict(bins=64, bin_us=1000, settle_bins=2, recent_bins=4, min_base_bins=8, ring_records_max=1 << 31),
               dict(group_cap=32768, bins=8192, ring_records_max=1)]
GOOD_CONFIGS = [dict(), dict(settle_bins=934), dict(bins=64, settle_bins=2, recent_bins=4, min_base_bins=58),
                dict(ring_records_max=17_592_186), dict(bins=64, bin_us=1000, settle_bins=2, recent_bins=4, min_base_bins=8, ring_records_max=(1 << 31) - 1),
                dict(bins=8192, bin_us=60_000_000, settle_bins=0, recent_bins=1, min_base_bins=1, ring_records_max=18325,
                     group_cap=1)]


def test_every_configuration_check_and_every_refused_step():
    for kw in BAD_CONFIGS:
        with pytest.raises(ValueError, match="load sli"):
            ld.LoadSliOracle(**kw)
    for kw in GOOD_CONFIGS:
        ld.LoadSliOracle(**kw)
    assert ld.default_ring_records_max(1024, 500_000) == 17_592_186 == (1 << 53) // (1024 * 500_000)
    assert ld.default_ring_records_max(64, 1000) == (1 << 31) - 1 and ld.LoadSliOracle().ring_records_max == 17_592_186
    o = ld.LoadSliOracle(**sc._cfg(64, span_cap=8))
    recs = np.ascontiguousarray(sc.traffic(0, sc.QH - 9, sc.QH - 6, 2, 0.25))
    a, cut = recs.ctypes.data, sc.cut_of(sc.QH)
    o.step_records(recs, cut, 3)
    before = o.resident()
    for bad in (lambda: o.step([(a, 63)], cut, 3), lambda: o.step_records(recs[:1], cut, 4), lambda: o.step_records(recs[:1], cut, -1),
                lambda: o.step_records(np.concatenate([recs, recs[:1]]), cut, 3), lambda: o.step([(0, 64)], cut, 3),
                lambda: o.step([(a, 8 * 64), (a, 64)], cut, 3), lambda: o.step_records(recs[:1], 0, 3),
                lambda: o.step_records(recs[:1], -7, 3)):
        with pytest.raises(ValueError, match="load sli step"):
            bad()
    sc.same_resident(o.resident(), before, "a refused step changes nothing")
    i = o.step([(a, 4 * 64), (a, 0), (0, 0), (a + 4 * 64, 4 * 64)], cut, 3)
    assert i == 1 and int(o.results(i, 3)["rows"]["arr_ring"][0]) == 16
    with pytest.raises(IndexError):
        o.results(-1, 3)
    with pytest.raises(IndexError):
        o.results(i - 3, 3)
    with pytest.raises(ValueError):
        o.results(i, 4)


# ---- the pipeline -------------------------------------------------------------------------------------

def _windows(rng, n_windows=6, G=3, per=16):
    """Windows of 16 bins each: finishing records of G services with durations up to 3 bins, first-token records
    beside them, one empty window."""
    wins, cuts = [], []
    for w in range(n_windows):
        qh = sc.Q0 + 7000 + per * (w + 1)
        n = 50
        start = (qh - rng.integers(1, per, n)) * sc.BIN + rng.integers(0, sc.BIN, n)
        recs = sc.reqs(rng.integers(0, G + 1, n), start, rng.integers(0, 24, n) * 0.125)
        recs["ttft_ms"] = rng.choice([100.0, 900.0], n).astype(F32)
        first = recs[:10].copy()
        first["flags"] = R.SPAN_FIRST_TOKEN
        wins.append(np.concatenate([recs, first]) if w != 3 else np.zeros(0, R.SPAN))
        cuts.append(sc.cut_of(qh))
    return wins, cuts


def test_pipeline_on_the_host_engine_carries_the_new_keys_only_when_switched_on():
    from llm_slo_ebpf_toolkit_amd.pipeline.window import WindowPipeline

    rng = np.random.default_rng(47)
    groups = [3, 3, 2, 3, 1, 3]
    wins, cuts = _windows(rng)
    cuts[4] = 0  # a cut without a time: skipped and counted
    off, none, _ = sc.run_pipeline("cpu", wins, cuts, groups, 0)
    onr, loads, skipped = sc.run_pipeline("cpu", wins, cuts, groups, 64)
    ref = ld.LoadSliOracle(**sc._cfg(64, group_cap=8, span_cap=1024))
    assert none == [] and skipped == 1
    for w, (a, b, d) in enumerate(zip(off, onr, loads)):
        assert not set(a) & set(ld.RESULT_KEYS) and set(b) == set(a) | set(ld.RESULT_KEYS)
        for key in a:
            assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), f"window {w} {key}"
        want = ld.empty_result(groups[w]) if w == 4 else ref.results(ref.step_records(wins[w], cuts[w], groups[w]), groups[w])
        sc.same_results(d, want, f"window {w}")
        for key, v in ld.result_keys(want).items():
            np.testing.assert_array_equal(b[key], v, err_msg=f"window {w} {key}")
    assert int(onr[5]["load_rows"]["arr_ring"].sum()) > 40 and int(onr[5]["load_stats"][0]) > 20
    with pytest.raises(ValueError, match="one GPU: no communicator, no sharding"):
        WindowPipeline(1024, 64, 4, engine="cpu", shard=(0, 2), load_sli=64)
    with pytest.raises(ValueError, match="load sli: bins"):
        WindowPipeline(1024, 64, 4, engine="cpu", load_sli=100)
    with pytest.raises(ValueError, match="must fit the ring's bins"):
        WindowPipeline(1024, 64, 4, engine="cpu", load_sli=64)  # 15 s of 500 ms bins three times over
    with pytest.raises(ValueError, match="load sli: factor_milli"):
        WindowPipeline(1024, 64, 4, engine="cpu", load_sli=1024, load_factor_milli=1000)
    p = WindowPipeline(1024, 64, 4, engine="cpu")
    try:
        assert p.load is None and p._no_side_tracker and p.load_skipped == 0
    finally:
        p.close()
    p = WindowPipeline(1024, 64, 4, engine="cpu", load_sli=1024)
    try:
        assert (p.load.bin_us, p.load.settle, p.load.recent, p.load.min_base_bins) == (500_000, 30, 30, 60)
        assert (p.load.f, p.load.min_requests, p.load.min_conc_milli) == (1500, 20, 1000)
        assert not p._no_side_tracker and not p.copy_ahead
    finally:
        p.close()


# ---- the agent ----------------------------------------------------------------------------------------

def _agent(tmp_path, tag, **kw):
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions

    log = tmp_path / f"decisions-{tag}.jsonl"
    o = AgentOptions(engine="cpu", source="replay", gpus=1, window_events=2048, window_spans=128, window_groups=8,
                     window_ms=300, metrics_bind="", output="stdout", ring_name=f"/mislo-ld-{tag}-{os.getpid()}",
                     config="", min_confidence=0.0, scenario="full", disable_overhead_guard=True,
                     decision_log=str(log), **kw)
    out = io.StringIO()
    a = Agent(o, out_stream=out)
    try:
        assert a.run_windows(max_windows=4) == 0
    finally:
        a.close()
    return a, [json.loads(ln) for ln in log.read_text().splitlines()], out.getvalue()


def test_agent_flags_defaults_and_what_is_refused():
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions
    from llm_slo_ebpf_toolkit_amd.cli.agent import parse

    fields = ("load_sli", "load_bin_ms", "load_bins", "load_settle_ms", "load_recent_ms", "load_factor", "load_min_requests",
              "load_min_concurrency")
    o, _ = parse(["--engine", "cpu", "--load-sli", "--load-bin-ms", "250", "--load-bins", "2048", "--load-settle-ms", "20000",
                  "--load-recent-ms", "10000", "--load-factor", "2", "--load-min-requests", "7", "--load-min-concurrency", "0.5"])
    assert tuple(getattr(o, f) for f in fields) == (True, 250.0, 2048, 20000.0, 10000.0, 2.0, 7, 0.5)
    d = parse([])[0]
    assert tuple(getattr(d, f) for f in fields) == (False, 0.0, 1024, 15000.0, 15000.0, 1.5, 20, 1.0)
    assert AgentOptions().load_sli is False
    kw = dict(engine="cpu", source="replay", config="", output="stdout", metrics_bind="")
    a = Agent(AgentOptions(ring_name=f"/mislo-ld2-{os.getpid()}", window_ms=2000, **kw))
    try:  # a quarter of the window; the millisecond flags become bins by ceil
        assert a.load_params() == dict(bin_us=500_000, settle_bins=30, recent_bins=30, min_base_bins=60, factor_milli=1500,
                                       min_requests=20, min_conc_milli=1000)
        a.check_load_flags()
    finally:
        a.close()
    a = Agent(AgentOptions(ring_name=f"/mislo-ld3-{os.getpid()}", window_ms=2, load_bin_ms=7.0, load_settle_ms=15.0,
                           load_recent_ms=7.001, load_bins=64, **kw))
    try:
        p = a.load_params()
        assert (p["bin_us"], p["settle_bins"], p["recent_bins"], p["min_base_bins"]) == (7000, 3, 2, 4)
    finally:
        a.close()
    a = Agent(AgentOptions(ring_name=f"/mislo-ld5-{os.getpid()}", window_ms=2, **kw))
    try:
        assert a.load_params()["bin_us"] == 1000, "at least 1 ms"
    finally:
        a.close()
    for extra, match in ((dict(gpus=2, load_sli=True), "--load-sli runs on one GPU"),
                         (dict(load_sli=True, load_bins=64), "--load-settle-ms 15000 .60 bins. .* --load-recent-ms 15000 .60 bins. .* --load-bins 64 at --load-bin-ms 250"),
                         (dict(load_sli=True, window_ms=100), "--load-settle-ms .* --load-bins 1024"),
                         (dict(load_sli=True, load_bins=1000), "bins must be a power of two.*--load-bins"),
                         (dict(load_sli=True, load_factor=1.0), "factor_milli.*--load-factor"),
                         (dict(load_sli=True, load_factor=65.0), "factor_milli.*--load-factor"),
                         (dict(load_sli=True, load_min_requests=0), "min_requests.*--load-min-requests"),
                         (dict(load_sli=True, load_min_concurrency=0.0), "min_conc_milli.*--load-min-concurrency"),
                         (dict(load_sli=True, load_bin_ms=70_000.0, load_settle_ms=0.0), "bin_us.*--load-bin-ms"),
                         (dict(load_sli=True, load_recent_ms=0.0), "--load-recent-ms > 0"),
                         (dict(load_sli=True, load_settle_ms=-1.0), "--load-settle-ms must be >= 0")):
        a = Agent(AgentOptions(ring_name=f"/mislo-ld4-{os.getpid()}", **{**kw, **extra}))
        try:
            with pytest.raises(ValueError, match=match):
                a.run_windows(max_windows=1)
        finally:
            a.close()


def _fabricated():
    """The slowdown case for service 0 ("rag"), nothing for service 1, a surge for service 2."""
    o = ld.LoadSliOracle(**sc._cfg(64))
    o.step_records(sc.EMPTY, sc.cut_of(sc.QF), 3)
    surge = np.concatenate([sc._spread(8, sc.BASE), sc._spread(6, sc.REC)])
    surge["group_id"] = 2
    i = o.step_records(sc.cat(sc.traffic(0, *sc.BASE, 2, 0.25), sc.traffic(0, *sc.REC, 2, 0.75), surge, sc.req(7, sc.QF, 0, 1.0)),
                       sc.cut_of(sc.QF + 13), 3)
    return ld.result_keys(o.results(i, 3)), ld.stats_dict(o.results(i, 3)["stats"])


def test_the_decision_log_entry_and_the_series_from_a_fabricated_result():
    from llm_slo_ebpf_toolkit_amd.agent.metrics import AgentMetrics
    from llm_slo_ebpf_toolkit_amd.export.prometheus import parse_exposition

    res, stats = _fabricated()
    e = [ld.summary(res["load_rows"][g], sc.BIN, sc.RECENT) for g in range(3)]
    for x in e:
        assert set(x) == {"state", "age_windows", "warming", "arrivals_per_s", "concurrency", "service_time_ms"}
        assert set(x["arrivals_per_s"]) == set(x["service_time_ms"]) == {"recent", "base"}
        assert set(x["concurrency"]) == {"recent", "base", "peak", "peak_ts_ns"}
    assert (e[0]["state"], e[0]["age_windows"], e[0]["warming"]) == ("slowdown", 1, False)
    assert e[0]["arrivals_per_s"] == {"recent": 2000.0, "base": 2000.0} and e[0]["concurrency"]["base"] == 0.5
    assert e[0]["service_time_ms"]["base"] == 0.25 and e[0]["service_time_ms"]["recent"] == round(5.75 / 7, 6)
    assert e[0]["concurrency"]["peak"] == 3 and e[0]["concurrency"]["peak_ts_ns"] == (sc.QF + 9) * sc.BIN * 1000
    assert e[1] == {"state": "steady", "age_windows": 0, "warming": False, "arrivals_per_s": {"recent": 0.0, "base": 0.0},
                    "concurrency": {"recent": 0.0, "base": 0.0, "peak": 0, "peak_ts_ns": None},
                    "service_time_ms": {"recent": None, "base": None}}
    assert e[2]["state"] == "surge" and e[2]["arrivals_per_s"] == {"recent": 1500.0, "base": 1000.0}
    assert e[2]["service_time_ms"] == {"recent": 0.0, "base": 0.0}
    json.dumps(e)
    assert stats["out_of_group"] == 1 and stats["observed"] == 16 + 8 + 14
    m = AgentMetrics("probe", "auto", [], [])
    for _ in range(2):
        m.observe_load(res, stats, ["rag", "chat"], sc.BIN, sc.RECENT)
    text = m.registry.exposition()
    v = parse_exposition(text)
    assert v['llm_slo_agent_load_state{service="rag"}'] == 2 and v['llm_slo_agent_load_state{service="chat"}'] == 0
    assert v['llm_slo_agent_load_state{service="group-2"}'] == 1
    assert v['llm_slo_agent_request_rate{service="rag",range="recent"}'] == 2000 == v['llm_slo_agent_request_rate{service="rag",range="base"}']
    assert v['llm_slo_agent_request_rate{service="group-2",range="recent"}'] == 1500
    assert v['llm_slo_agent_concurrency{service="rag",range="base"}'] == 0.5 and v['llm_slo_agent_concurrency{service="rag",range="peak"}'] == 3
    assert 1.4 < v['llm_slo_agent_concurrency{service="rag",range="recent"}'] <= 1.5
    for reason in ld.EVENT_STATS:
        assert v[f'llm_slo_agent_load_events_total{{reason="{reason}"}}'] == 2 * stats[reason]
    assert 'reason="observed"' not in text
    # a warming row sets the state and the peak and keeps the ranges' last values
    m.observe_load({"load_rows": ld.warming_rows(1)}, dict.fromkeys(ld.STATS, 0), ["rag"], sc.BIN, sc.RECENT)
    v = parse_exposition(m.registry.exposition())
    assert v['llm_slo_agent_load_state{service="rag"}'] == 4 and v['llm_slo_agent_request_rate{service="rag",range="recent"}'] == 2000


@pytest.mark.timeout(120)
def test_the_agent_logs_a_load_entry_per_scored_group_and_off_means_nothing_new(tmp_path):
    from llm_slo_ebpf_toolkit_amd.contracts import validator

    a, rows, out = _agent(tmp_path, "on", load_sli=True, load_bins=64, load_settle_ms=150.0, load_recent_ms=300.0)
    assert rows and all("load" in r for r in rows)
    assert a.specs[0].load_sli == 64 and dict(a.specs[0].load_params) == dict(
        bin_us=75_000, settle_bins=2, recent_bins=4, min_base_bins=8, factor_milli=1500, min_requests=20, min_conc_milli=1000)
    keys = {"state", "age_windows", "warming", "arrivals_per_s", "concurrency", "service_time_ms"}
    assert all(set(r["load"]) == keys and r["load"]["state"] in ld.STATE_NAMES for r in rows)
    assert all(list(r)[-1] == "why" for r in rows)
    emitted = [json.loads(ln) for ln in out.splitlines() if ln.startswith('{"incident_id"')]
    assert emitted
    for d in emitted:
        assert "load" not in d
        validator.validate("incident-attribution", d)
    text = a.metrics.registry.exposition()
    assert "llm_slo_agent_load_state{" in text and 'llm_slo_agent_load_events_total{reason="too_old"}' in text
    b, rows_off, out_off = _agent(tmp_path, "off")
    assert b.specs[0].load_sli == 0 and b.specs[0].load_params == () and all("load" not in r for r in rows_off)
    for series in ("llm_slo_agent_load_state{", "llm_slo_agent_request_rate{", "llm_slo_agent_concurrency{",
                   "llm_slo_agent_load_events_total{"):
        assert series not in b.metrics.registry.exposition()
    # the replay is cut by the wall clock, so two runs need not see the same windows: the shapes are compared
    off = [json.loads(ln) for ln in out_off.splitlines() if ln.startswith('{"incident_id"')]
    assert off and {frozenset(d) for d in off} == {frozenset(d) for d in emitted}, "emitted incidents keep their fields"
    assert {frozenset(r) | {"load"} for r in rows_off} == {frozenset(r) for r in rows}
    assert {r["why"] for r in rows} <= {"emitted", "low_confidence", "no_burn", "recovered"}


# ---- the tracker's host side under the host sanitizers ------------------------------------------------

def test_loadsli_host_side_under_address_and_ub_sanitizers(tmp_path):
    """ops/csrc/loadsli_host.h (the duration rule, the placement, the scan by lanes against the recurrence, the
    ranges, the three compares against unsigned __int128 at the bounds' extremes, argument checks, layout, the
    population bound) needs no device: a stand-alone program over it, built with AddressSanitizer + UBSan, run as a
    child process. It prints the durations and the layout of several group counts, which must be the Python mirror's."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "llm_slo_ebpf_toolkit_amd", "ops", "csrc")
    exe = tmp_path / "loadsli_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-Wall", "-Werror", f"-I{csrc}", os.path.join(root, "tests", "native", "loadsli_host_check.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "loadsli host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
    durs = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("dur ")]
    assert len(durs) == len(sc.DUR_PATTERNS)
    for (x, want), (bits, got) in zip(sc.DUR_PATTERNS, durs):
        assert float.fromhex(bits) == float(F32(x)) and int(got) == want == int(ld.dur_us(F32(x)))
    got = [tuple(int(x) for x in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("layout ")]
    assert len(got) == 7
    for g, *at in got:
        off = ld.layout(g)
        assert at == [off[k] for k in ("rows", "stats", "words")]
    dev, = [int(ln.split()[1]) for ln in r.stdout.splitlines() if ln.startswith("device_bytes ")]
    assert dev == ld.device_bytes(1024, 16384, 64)
    cap, = [int(ln.split()[1]) for ln in r.stdout.splitlines() if ln.startswith("ring_records_max ")]
    assert cap == ld.default_ring_records_max(1024, 500_000)
