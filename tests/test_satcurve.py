"""The saturation curve on the host (pipeline/satcurve.py): the oracle against a per-request, per-bin
brute force on every named case and on seeded random runs, with the in-flight invariants; the level and
the knee rules; every configuration check and refused step; the pipeline on the host engine (the new keys
only when switched on, every other key byte-equal); the agent's flags and refusals, the decision log
entry and the series; the other oracles unaffected; and the tracker's host side under the host
sanitizers. No GPU."""

import io
import json
import os

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.pipeline import loadsli as ld
from llm_slo_ebpf_toolkit_amd.pipeline import satcurve as sat
from tests import satcurve_scenarios as sc

F32 = np.float32


# ---- the rules ------------------------------------------------------------------------------------------

def _brute_run(c, seen_stats=None):
    ref, br = sat.SaturationOracle(**c.cfg), sc.Brute(**c.cfg)
    res, resid = [], []
    for w, (recs, cut, G) in enumerate(c.steps):
        what = f"{c.name} step {w}"
        if w in c.refused:
            before = ref.resident()
            with pytest.raises(ValueError, match=c.refused[w]):
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
        assert (busy >= 0).all() and (busy <= active * ref.bin_us).all() and (now["carry"] >= 0).all(), what
        # a bin's sli counts at most its starts, its breaches at most its requests
        n, b = now["sli"] & np.uint64(0xFFFFFFFF), now["sli"] >> np.uint64(32)
        assert (b <= n).all() and (n <= (now["counts"] & np.uint64(0xFFFFFFFF))).all(), what
        assert (now["gen"][..., 1] <= now["gen"][..., 0]).all(), what
        # the block is the rows, the curve and the statistics, every array on 16 bytes
        lay, block = sat.layout(ref.group_cap), ref.block(i)
        assert block.dtype == np.uint32 and len(block) == lay["words"]
        assert lay["curve"] * 4 % 16 == 0 and lay["stats"] * 4 % 16 == 0 and lay["words"] % 4 == 0
        assert block[:lay["curve"]].tobytes() == a["rows"].tobytes()
        assert block[lay["curve"]:lay["stats"]].tobytes() == a["curve"].tobytes()
        assert block[lay["stats"]:][:8].tolist() == a["stats"].tolist()
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
    seen = np.zeros(sat.N_STATS, np.int64)
    states, knees = set(), 0
    for seed in range(6):
        for r in _brute_run(sc._random(f"random seed {seed}", 3 if seed % 2 else 2, 100 + seed, 16, 150,
                                       epoch_bins=64 if seed % 2 else 128), seen):
            states.update(r["rows"]["state"].tolist())
            knees += int((r["rows"]["knee_level"] != sat.NONE).sum())
    assert (seen > 0).all(), dict(zip(sat.STATS, seen.tolist()))
    assert states == {sat.UNKNOWN, sat.NO_KNEE, sat.BELOW, sat.SATURATED} and knees > 10, (states, knees)


def test_the_named_cases_cover_the_list():
    names = " | ".join(sc.CASE_NAMES)
    for word in ("inside one bin", "across three bins", "on a bin's edge", "clipped", "clipped without a ttft", "too old",
                 "future start", "future start without a ttft", "future end", "no time", "invalid latencies", "out of group",
                 "skipped", "no-sli finishing", "ttft validity", "without a ttft occupies", "u = 15", "u = 16", "u = 17",
                 "u = 8191", "above u = 8191", "advance by 0", "B or more", "moving back", "exactly at q_first",
                 "changes an unevicted bin's level", "start bin is evicted", "epoch boundary crossed", "dropped after two epochs",
                 "more than two epochs", "clean step curve", "noisy low level", "equal maxima", "exactly 0",
                 "n_knee at min_requests", "one below min_requests", "budget compare at equality", "four states and age",
                 "ring_records_max", "curve_records_max", "hot one bin", "hot four bins"):
        assert word in names, word
    for c in sc.cases():
        assert c.cfg["bins"] == 64 and c.cfg["bin_us"] == 1000 and c.cfg["group_cap"] <= 5 and c.cfg["epoch_bins"] in (64, 128)
        assert all(len(recs) <= c.cfg["span_cap"] for recs, _, _ in c.steps), c.name
    assert all(len(sc.case(n).steps[-1][0]) == 4096 for n in sc.CASE_NAMES if n.startswith("hot"))


def test_level_knee_state_helpers_and_the_summary():
    u = np.arange(sat.MAX_U + 1)
    level = sat.level_of_u(u)
    assert level.min() == 0 and level.max() == sat.K - 1 == 159 and (np.diff(level) >= 0).all() and (np.diff(level) <= 1).all()
    assert (level[:16] == u[:16]).all() and len(np.unique(level)) == sat.K
    assert (sat.level_of_u(sat.lower(np.arange(sat.K))) == np.arange(sat.K)).all() and int(sat.lower(sat.K)) == sat.MAX_U + 1
    assert [int(sat.level_of_u(x)) for x in (15, 16, 17, 31, 32, 33, 8191)] == [15, 16, 17, 31, 32, 32, 159]
    assert sat.u_of([1874, 1875, 2000, 1023875, 2_000_000, 0, -4], 1000).tolist() == [14, 15, 16, 8191, 8191, 0, 0]
    assert int(sat.u_of(1 << 53, 1000)) == sat.MAX_U
    assert sat.concurrency_of(15) == 15 / 8 and sat.concurrency_of(16) == 2.0 and sat.concurrency_of(32) == 4.0
    curve = np.zeros((sat.K, 2), np.uint64)
    assert sat.knee_of(curve, 100_000, 1) == (sat.NONE, 0, 0, False)
    curve[40] = (10, 1)
    assert sat.knee_of(curve, 100_000, 1)[0] == sat.NONE and sat.knee_of(curve, 99_999, 1) == (40, 10, 1, True)
    curve[80], curve[60], curve[20] = (8, 2), (4, 0), (6, 1)  # S = 12 at 80 and again at 20: the larger level
    assert sat.knee_of(curve, 100_000, 8) == (80, 8, 2, True) and sat.knee_of(curve, 100_000, 9) == (80, 8, 2, False)
    top = np.zeros((sat.K, 2), np.uint64)
    top[159] = (1 << 40, 1 << 40)
    assert sat.knee_of(top, 1, 1) == (159, 1 << 40, 1 << 40, True)
    assert [sat.state_of(*x) for x in ((False, 9, 4, True, 9, 5), (True, 3, 4, True, 9, 5), (True, 4, 4, False, 9, sat.NONE),
                                       (True, 4, 4, True, 4, 5), (True, 4, 4, True, 5, 5))] == [0, 0, 1, 2, 3]
    assert [sat.age_of(*x) for x in ((3, 0), (3, 7), (3, 2 ** 32 - 1), (2, 7), (0, 7))] == [1, 8, 2 ** 32 - 1, 0, 0]
    assert sat.fold_of(-1, 500, -1, 64) == (0, 0, 0, -1) and sat.fold_of(500, 500, 500, 64) == (0, 0, 0, -1)
    assert sat.fold_of(563, 565, 500, 64) == (500, 2, 500, 501) and sat.fold_of(562, 564, 500, 64) == (499, 2, 500, 500)
    assert sat.fold_of(570, 1000, 500, 64) == (507, 64, 507, 570)
    assert sat.budget_ppm(0.99) == 10_000
    row = np.zeros(1, sat.SAT_ROW)[0]
    row["state"], row["age"], row["knee_level"], row["recent_u"], row["top_level"] = sat.BELOW, 0, 48, 20, 50
    row["n_total"], row["b_total"], row["n_knee"], row["b_knee"] = 40, 9, 16, 8
    curve = np.zeros((sat.K, 2), np.uint64)
    curve[16], curve[48], curve[50] = (24, 1), (10, 4), (6, 4)
    assert sat.summary(row, curve) == {
        "state": "below", "age_windows": 0, "knee_concurrency": 8.0, "recent_concurrency": 2.5, "headroom": 3.2,
        "requests": 40, "breaches": 9, "at_knee": {"requests": 16, "breaches": 8},
        "curve": [{"concurrency": 2.0, "requests": 24, "breaches": 1}, {"concurrency": 8.0, "requests": 10, "breaches": 4},
                  {"concurrency": 9.0, "requests": 6, "breaches": 4}]}
    e = sat.summary(sat.unknown_rows(1)[0], np.zeros((sat.K, 2), np.uint64))
    assert e == {"state": "unknown", "age_windows": 0, "knee_concurrency": None, "recent_concurrency": None, "headroom": None,
                 "requests": 0, "breaches": 0, "at_knee": {"requests": None, "breaches": None}, "curve": []}
    row["recent_u"] = 0  # an idle service below a knee: no headroom to quote
    assert sat.summary(row, curve)["headroom"] is None and sat.summary(row, curve)["recent_concurrency"] == 0.0
    json.dumps(e)
    assert sat.empty_result(3)["rows"].tobytes() == sat.unknown_rows(3).tobytes() and not sat.empty_result(3)["stats"].any()
    assert set(sat.result_keys(sat.empty_result(2))) == set(sat.RESULT_KEYS) == {"sat_rows", "sat_curve", "sat_stats"}


BAD_CONFIGS = [dict(bins=32), dict(bins=16384), dict(bins=96), dict(bin_us=999), dict(bin_us=60_000_001),
               dict(settle_bins=-1), dict(recent_bins=0), dict(settle_bins=995), dict(bins=64, epoch_bins=64, settle_bins=61, recent_bins=4),
               dict(epoch_bins=1023), dict(epoch_bins=1 << 31), dict(budget_ppm=0), dict(budget_ppm=1_000_000),
               dict(min_requests=0), dict(min_requests=1 << 31), dict(slo_ms=-1.0), dict(slo_ms=float("nan")),
               dict(group_cap=0), dict(group_cap=65537), dict(span_cap=0), dict(n_buffers=0), dict(n_buffers=65),
               dict(ring_records_max=0), dict(ring_records_max=17_592_187), dict(curve_records_max=0),
               dict(curve_records_max=(1 << 40) + 1), dict(group_cap=16384, bins=8192, epoch_bins=8192, ring_records_max=1)]
GOOD_CONFIGS = [dict(), dict(settle_bins=994), dict(bins=64, epoch_bins=64, settle_bins=60, recent_bins=4), dict(epoch_bins=1024),
                dict(epoch_bins=(1 << 31) - 1), dict(budget_ppm=1), dict(budget_ppm=999_999), dict(curve_records_max=1),
                dict(bins=8192, bin_us=60_000_000, epoch_bins=8192, settle_bins=0, recent_bins=1, ring_records_max=18325,
                     group_cap=1)]


def test_every_configuration_check_and_every_refused_step():
    for kw in BAD_CONFIGS:
        with pytest.raises(ValueError, match="saturation curve"):
            sat.SaturationOracle(**kw)
    for kw in GOOD_CONFIGS:
        sat.SaturationOracle(**kw)
    o = sat.SaturationOracle()
    assert (o.ring_records_max, o.curve_records_max) == (17_592_186, 1 << 40)
    assert sat.layout(64) == {"rows": 0, "curve": 1024, "stats": 41984, "words": 41992}
    assert sat.device_bytes(1024, 16384, 64) == 16384 * 64 + 64 * 1024 * 24 + 64 * 8 + 64 * 2 * 160 * 16 + 41992 * 4
    o = sat.SaturationOracle(**sc._cfg(span_cap=8))
    recs = np.ascontiguousarray(sc.traffic(0, sc.QF - 9, sc.QF - 6, 2, 0.25))
    a, cut = recs.ctypes.data, sc.cut_of(sc.QF)
    o.step_records(recs, cut, 3)
    before = o.resident()
    for bad in (lambda: o.step([(a, 63)], cut, 3), lambda: o.step_records(recs[:1], cut, 4), lambda: o.step_records(recs[:1], cut, -1),
                lambda: o.step_records(np.concatenate([recs, recs[:1]]), cut, 3), lambda: o.step([(0, 64)], cut, 3),
                lambda: o.step([(a, 8 * 64), (a, 64)], cut, 3), lambda: o.step_records(recs[:1], 0, 3),
                lambda: o.step_records(recs[:1], -7, 3)):
        with pytest.raises(ValueError, match="saturation curve step"):
            bad()
    sc.same_resident(o.resident(), before, "a refused step changes nothing")
    i = o.step([(a, 4 * 64), (a, 0), (0, 0), (a + 4 * 64, 4 * 64)], cut, 3)
    assert i == 1 and int(o.resident()["sli"].sum()) == 16
    with pytest.raises(IndexError):
        o.results(-1, 3)
    with pytest.raises(IndexError):
        o.results(i - 3, 3)
    with pytest.raises(ValueError):
        o.results(i, 4)


# ---- the pipeline -------------------------------------------------------------------------------------

def _windows(rng, n_windows=6, G=3, per=16):
    """Windows of 16 bins each: finishing records of G services with durations up to 3 bins and a TTFT that
    breaches more often the longer the request, some without a TTFT, first-token records beside them, one empty
    window."""
    wins, cuts = [], []
    for w in range(n_windows):
        qh = sc.Q0 + 7040 + per * (w + 1)
        n = 50
        start = (qh - rng.integers(1, per, n)) * sc.BIN + rng.integers(0, sc.BIN, n)
        dur = rng.integers(0, 24, n)
        ttft = np.where(rng.random(n) < 0.1, np.nan, np.where(rng.random(n) < dur / 30.0, sc.BREACH, sc.OK))
        recs = sc.reqs(rng.integers(0, G + 1, n), start, dur * 0.125, ttft)
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
    onr, sats, skipped = sc.run_pipeline("cpu", wins, cuts, groups, 64)
    ref = sat.SaturationOracle(**sc._cfg(group_cap=8, span_cap=1024, budget_ppm=150_000))
    assert none == [] and skipped == 1
    for w, (a, b, d) in enumerate(zip(off, onr, sats)):
        assert not set(a) & set(sat.RESULT_KEYS) and set(b) == set(a) | set(sat.RESULT_KEYS)
        for key in a:
            assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), f"window {w} {key}"
        want = sat.empty_result(groups[w]) if w == 4 else ref.results(ref.step_records(wins[w], cuts[w], groups[w]), groups[w])
        sc.same_results(d, want, f"window {w}")
        for key, v in sat.result_keys(want).items():
            np.testing.assert_array_equal(b[key], v, err_msg=f"window {w} {key}")
    assert int(onr[5]["sat_rows"]["n_total"].sum()) > 40 and int(onr[5]["sat_stats"][0]) > 20
    assert int(onr[5]["sat_stats"][sat.STATS.index("no_ttft")]) > 0
    with pytest.raises(ValueError, match="one GPU: no communicator, no sharding"):
        WindowPipeline(1024, 64, 4, engine="cpu", shard=(0, 2), saturation=64)
    with pytest.raises(ValueError, match="saturation curve: bins"):
        WindowPipeline(1024, 64, 4, engine="cpu", saturation=100)
    with pytest.raises(ValueError, match="settle_bins \\+ recent_bins must fit"):
        WindowPipeline(1024, 64, 4, engine="cpu", saturation=64, sat_settle_bins=40, sat_recent_bins=25)
    with pytest.raises(ValueError, match="saturation curve: epoch_bins"):
        WindowPipeline(1024, 64, 4, engine="cpu", saturation=1024, sat_epoch_bins=1000)
    p = WindowPipeline(1024, 64, 4, engine="cpu")
    try:
        assert p.sat is None and p._no_side_tracker and p.sat_skipped == 0
    finally:
        p.close()
    p = WindowPipeline(1024, 64, 4, engine="cpu", saturation=1024, ttft_slo_ms=650.0)
    try:
        assert (p.sat.bin_us, p.sat.settle, p.sat.recent, p.sat.epoch_bins) == (500_000, 30, 30, 43_200)
        assert (p.sat.budget_ppm, p.sat.min_requests, float(p.sat.slo)) == (10_000, 200, 650.0)
        assert not p._no_side_tracker and not p.copy_ahead
    finally:
        p.close()


def test_the_other_oracles_are_unaffected_by_the_tracker_beside_them():
    """The load SLI beside the saturation curve over the same windows: its results are those of a run alone."""
    rng = np.random.default_rng(48)
    wins, cuts = _windows(rng)
    lkw = dict(load_sli=64, load_bin_us=sc.BIN, load_settle_bins=2, load_recent_bins=4, load_min_base_bins=8)
    both, _, _ = sc.run_pipeline("cpu", wins, cuts, 3, 64, **lkw)
    alone, _, _ = sc.run_pipeline("cpu", wins, cuts, 3, 0, **lkw)
    for w, (a, b) in enumerate(zip(both, alone)):
        assert set(a) == set(b) | set(sat.RESULT_KEYS) and "load_rows" in b
        for key in b:
            assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), f"window {w} {key}"


# ---- the agent ----------------------------------------------------------------------------------------

def _agent(tmp_path, tag, **kw):
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions

    log = tmp_path / f"decisions-{tag}.jsonl"
    o = AgentOptions(engine="cpu", source="replay", gpus=1, window_events=2048, window_spans=128, window_groups=8,
                     window_ms=300, metrics_bind="", output="stdout", ring_name=f"/mislo-sat-{tag}-{os.getpid()}",
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

    fields = ("saturation_curve", "sat_bin_ms", "sat_bins", "sat_settle_ms", "sat_recent_ms", "sat_epoch_s", "sat_min_requests")
    o, _ = parse(["--engine", "cpu", "--saturation-curve", "--sat-bin-ms", "250", "--sat-bins", "2048", "--sat-settle-ms", "20000",
                  "--sat-recent-ms", "10000", "--sat-epoch-s", "3600", "--sat-min-requests", "70"])
    assert tuple(getattr(o, f) for f in fields) == (True, 250.0, 2048, 20000.0, 10000.0, 3600.0, 70)
    d = parse([])[0]
    assert tuple(getattr(d, f) for f in fields) == (False, 0.0, 1024, 15000.0, 15000.0, 21600.0, 200)
    assert AgentOptions().saturation_curve is False
    kw = dict(engine="cpu", source="replay", config="", output="stdout", metrics_bind="")
    a = Agent(AgentOptions(ring_name=f"/mislo-sat2-{os.getpid()}", window_ms=2000, **kw))
    try:  # a quarter of the window; the millisecond flags become bins by ceil; the budget of slo_target 0.99
        assert a.saturation_params() == dict(bin_us=500_000, settle_bins=30, recent_bins=30, epoch_bins=43_200,
                                             budget_ppm=10_000, min_requests=200)
        a.check_saturation_flags()
    finally:
        a.close()
    a = Agent(AgentOptions(ring_name=f"/mislo-sat3-{os.getpid()}", window_ms=2, sat_bin_ms=7.0, sat_settle_ms=15.0,
                           sat_recent_ms=7.001, sat_epoch_s=0.5, sat_bins=64, slo_target=0.95, **kw))
    try:
        p = a.saturation_params()
        assert (p["bin_us"], p["settle_bins"], p["recent_bins"], p["epoch_bins"], p["budget_ppm"]) == (7000, 3, 2, 72, 50_000)
        a.check_saturation_flags()
    finally:
        a.close()
    a = Agent(AgentOptions(ring_name=f"/mislo-sat5-{os.getpid()}", window_ms=2, **kw))
    try:
        assert a.saturation_params()["bin_us"] == 1000, "at least 1 ms"
    finally:
        a.close()
    on = dict(saturation_curve=True)
    for extra, match in ((dict(gpus=2, **on), "--saturation-curve runs on one GPU"),
                         (dict(sat_bins=64, **on), "--sat-settle-ms 15000 .60 bins. . --sat-recent-ms 15000 .60 bins. do not fit "
                                                   "--sat-bins 64 at --sat-bin-ms 250"),
                         (dict(window_ms=100, **on), "--sat-settle-ms .* --sat-bins 1024"),
                         (dict(sat_epoch_s=200.0, **on), "--sat-epoch-s 200 .800 bins. is shorter than the ring: --sat-bins 1024"),
                         (dict(sat_bins=1000, **on), "bins must be a power of two.*--sat-bins"),
                         (dict(sat_min_requests=0, **on), "min_requests.*--sat-min-requests"),
                         (dict(sat_bin_ms=70_000.0, sat_settle_ms=0.0, sat_epoch_s=172_800.0, **on), "bin_us.*--sat-bin-ms"),
                         (dict(sat_recent_ms=0.0, **on), "--sat-recent-ms > 0"),
                         (dict(sat_epoch_s=0.0, **on), "--sat-epoch-s > 0"),
                         (dict(sat_settle_ms=-1.0, **on), "--sat-settle-ms must be >= 0")):
        a = Agent(AgentOptions(ring_name=f"/mislo-sat4-{os.getpid()}", **{**kw, **extra}))
        try:
            with pytest.raises(ValueError, match=match):
                a.run_windows(max_windows=1)
        finally:
            a.close()


def _fabricated():
    """Service 0 ("rag") saturated at a knee of 8, nothing over budget for service 1, nothing at all for service 2."""
    o = sat.SaturationOracle(**sc._cfg())
    o.step_records(sc.EMPTY, sc.cut_of(sc.QF), 3)
    q = sc.QF
    recs = sc.cat(sc.full(0, q, 2, 0, 3), sc.full(0, q + 3, 4, 0, 2), sc.full(0, q + 8, 8, 4, 4), sc.full(1, q + 2, 5, 0, 2),
                  sc.req(7, q, 0, 1.0), sc.req(1, q + 1, 0, 0.5, np.nan))
    i = o.step_records(recs, sc.cut_of(q + 13), 3)
    return sat.result_keys(o.results(i, 3)), sat.stats_dict(o.results(i, 3)["stats"])


def test_the_decision_log_entry_and_the_series_from_a_fabricated_result():
    from llm_slo_ebpf_toolkit_amd.agent.metrics import AgentMetrics
    from llm_slo_ebpf_toolkit_amd.export.prometheus import parse_exposition

    res, stats = _fabricated()
    e = [sat.summary(res["sat_rows"][g], res["sat_curve"][g]) for g in range(3)]
    for x in e:
        assert list(x) == ["state", "age_windows", "knee_concurrency", "recent_concurrency", "headroom", "requests", "breaches",
                           "at_knee", "curve"]
        assert set(x["at_knee"]) == {"requests", "breaches"}
        assert all(set(c) == {"concurrency", "requests", "breaches"} for c in x["curve"])
    assert e[0] == {"state": "saturated", "age_windows": 1, "knee_concurrency": 8.0, "recent_concurrency": 8.0, "headroom": 1.0,
                    "requests": 46, "breaches": 16, "at_knee": {"requests": 32, "breaches": 16},
                    "curve": [{"concurrency": 2.0, "requests": 6, "breaches": 0}, {"concurrency": 4.0, "requests": 8, "breaches": 0},
                              {"concurrency": 8.0, "requests": 32, "breaches": 16}]}
    assert (e[1]["state"], e[1]["knee_concurrency"], e[1]["recent_concurrency"], e[1]["headroom"]) == ("no_knee", None, 0.0, None)
    assert e[1]["requests"] == 10 and e[1]["at_knee"] == {"requests": None, "breaches": None}
    assert e[2]["state"] == "unknown" and e[2]["curve"] == [] and e[2]["recent_concurrency"] is None
    json.dumps(e)
    assert stats["out_of_group"] == 1 and stats["no_ttft"] == 1 and stats["observed"] == 46 + 10 + 1
    m = AgentMetrics("probe", "auto", [], [])
    for _ in range(2):
        m.observe_saturation(res, stats, ["rag", "chat"])
    text = m.registry.exposition()
    v = parse_exposition(text)
    assert v['llm_slo_agent_saturation_state{service="rag"}'] == 3 and v['llm_slo_agent_saturation_state{service="chat"}'] == 1
    assert v['llm_slo_agent_saturation_state{service="group-2"}'] == 0
    assert v['llm_slo_agent_saturation_knee_concurrency{service="rag"}'] == 8
    assert v['llm_slo_agent_saturation_headroom_ratio{service="rag"}'] == 1
    assert 'saturation_knee_concurrency{service="chat"}' not in text
    for reason in sat.EVENT_STATS:
        assert v[f'llm_slo_agent_saturation_events_total{{reason="{reason}"}}'] == 2 * stats[reason]
    assert 'saturation_events_total{reason="observed"}' not in text
    # a row without a knee sets the state and keeps the knee's and the headroom's last values
    m.observe_saturation({"sat_rows": sat.unknown_rows(1), "sat_curve": np.zeros((1, sat.K, 2), np.uint64)},
                         dict.fromkeys(sat.STATS, 0), ["rag"])
    v = parse_exposition(m.registry.exposition())
    assert v['llm_slo_agent_saturation_state{service="rag"}'] == 0
    assert v['llm_slo_agent_saturation_knee_concurrency{service="rag"}'] == 8


@pytest.mark.timeout(120)
def test_the_agent_logs_a_saturation_entry_per_scored_group_and_off_means_nothing_new(tmp_path):
    from llm_slo_ebpf_toolkit_amd.contracts import validator

    a, rows, out = _agent(tmp_path, "on", saturation_curve=True, sat_bins=64, sat_settle_ms=150.0, sat_recent_ms=300.0,
                          sat_epoch_s=6.0, sat_min_requests=5)
    assert rows and all("saturation" in r for r in rows)
    assert a.specs[0].saturation == 64 and dict(a.specs[0].sat_params) == dict(
        bin_us=75_000, settle_bins=2, recent_bins=4, epoch_bins=80, budget_ppm=10_000, min_requests=5)
    keys = {"state", "age_windows", "knee_concurrency", "recent_concurrency", "headroom", "requests", "breaches", "at_knee",
            "curve"}
    assert all(set(r["saturation"]) == keys and r["saturation"]["state"] in sat.STATE_NAMES for r in rows)
    assert all(list(r)[-1] == "why" for r in rows)
    emitted = [json.loads(ln) for ln in out.splitlines() if ln.startswith('{"incident_id"')]
    assert emitted
    for d in emitted:
        assert "saturation" not in d
        validator.validate("incident-attribution", d)
    text = a.metrics.registry.exposition()
    assert "llm_slo_agent_saturation_state{" in text and 'llm_slo_agent_saturation_events_total{reason="no_ttft"}' in text
    b, rows_off, out_off = _agent(tmp_path, "off")
    assert b.specs[0].saturation == 0 and b.specs[0].sat_params == () and all("saturation" not in r for r in rows_off)
    for series in ("llm_slo_agent_saturation_state{", "llm_slo_agent_saturation_knee_concurrency{",
                   "llm_slo_agent_saturation_headroom_ratio{", "llm_slo_agent_saturation_events_total{"):
        assert series not in b.metrics.registry.exposition()
    # the replay is cut by the wall clock, so two runs need not see the same windows: the shapes are compared
    off = [json.loads(ln) for ln in out_off.splitlines() if ln.startswith('{"incident_id"')]
    assert off and {frozenset(d) for d in off} == {frozenset(d) for d in emitted}, "emitted incidents keep their fields"
    assert {frozenset(r) | {"saturation"} for r in rows_off} == {frozenset(r) for r in rows}
    assert {r["why"] for r in rows} <= {"emitted", "low_confidence", "no_burn", "recovered"}


def test_flag_off_nothing_is_constructed_and_the_merged_results_keep_their_bytes():
    """With the flag off the worker's spec asks for no tracker, and the controller's merge of the workers' results is
    the same bytes with and without the tracker's keys beside them (the replay agent is cut by the wall clock, so two
    agent runs are compared by shape above, not by bytes)."""
    import dataclasses

    from llm_slo_ebpf_toolkit_amd.agent.worker import WorkerSpec, merge_results

    defaults = {f.name: f.default for f in dataclasses.fields(WorkerSpec)}
    assert defaults["saturation"] == 0 and defaults["sat_params"] == ()
    res, _ = _fabricated()
    base = {"post": np.arange(48, dtype=np.float32).reshape(3, 16), "conf": np.arange(3, dtype=np.float32)}
    merged = merge_results([dict(base)], 3)
    assert set(merged) == set(base), "nothing of the tracker without its keys"
    with_keys = merge_results([dict(base, **{k: res[k] for k in ("sat_rows", "sat_curve")})], 3)
    assert set(with_keys) == set(base) | {"sat_rows", "sat_curve"}
    for key in base:
        assert np.asarray(with_keys[key]).tobytes() == np.asarray(merged[key]).tobytes() == base[key].tobytes()
    assert with_keys["sat_rows"].tobytes() == res["sat_rows"].tobytes()
    assert with_keys["sat_curve"].tobytes() == res["sat_curve"].tobytes()


# ---- the tracker's host side under the host sanitizers ------------------------------------------------

def test_satcurve_host_side_under_address_and_ub_sanitizers(tmp_path):
    """ops/csrc/satcurve_host.h (the placement, the level rule over every u against lower(), the fold's order by
    lanes against the recurrence, the generations, the knee against __int128 at the bounds' extremes, state, age,
    argument checks, layout, both population bounds) needs no device: a stand-alone program over it, built with
    AddressSanitizer + UBSan, run as a child process. It prints levels and the layout of several group counts,
    which must be the Python mirror's."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "llm_slo_ebpf_toolkit_amd", "ops", "csrc")
    exe = tmp_path / "satcurve_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-Wall", "-Werror", f"-I{csrc}", os.path.join(root, "tests", "native", "satcurve_host_check.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "satcurve host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
    levels = [tuple(int(x) for x in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("level ")]
    assert len(levels) == 3
    for b, u, l37, ltop in levels:
        assert (u, l37, ltop) == (int(sat.u_of(b * 3 // 2, b)), int(sat.level_of_u(sat.u_of(b * 37, b))),
                                  int(sat.level_of_u(sat.u_of(b * 2000, b))))
    got = [tuple(int(x) for x in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("layout ")]
    assert len(got) == 7
    for g, *at in got:
        off = sat.layout(g)
        assert at == [off[k] for k in ("rows", "curve", "stats", "words")]
    dev, = [int(ln.split()[1]) for ln in r.stdout.splitlines() if ln.startswith("device_bytes ")]
    assert dev == sat.device_bytes(1024, 16384, 64)
    cap, = [int(ln.split()[1]) for ln in r.stdout.splitlines() if ln.startswith("curve_records_max ")]
    assert cap == sat.MAX_CURVE_RECORDS
