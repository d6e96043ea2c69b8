"""The breach-onset tracker's rules on the host (pipeline/onset.py): the numpy oracle against a brute-force
loop over a dict of bins, every named case (tests/onset_scenarios.py CASES: the edges, zeros on a lane's
bins, the alarm threshold, clipped, quiet, wrap, jumping cuts, late records, step shapes), the scan by
prefix sums against the recurrence, every refusal, the ring bound's two sides, the host engine's result
keys, the agent's decision-log entry and series, and the tracker's host side (ops/csrc/onset_host.h)
under the host sanitizers. The device tracker against the oracle: tests/test_onset_gpu.py."""

import io
import json
import os

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.pipeline import onset as on
from tests import onset_scenarios as sc


def _oracle(cfg, **kw):
    return on.OnsetOracle(**dict(cfg, **kw))


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_oracle_equals_the_brute_force_after_every_step(name):
    c = sc.case(name)
    o, brute = _oracle(c.cfg), sc.Brute(**c.cfg)
    C = c.cfg["group_cap"]
    seen = []
    for w, (recs, cut, G) in enumerate(c.steps):
        want = brute.step(recs, cut, G)
        got = o.results(o.step_records(recs, cut, G), C)
        sc.same_results(got, want, f"{name} step {w}")
        sc.same_resident(o.resident(), brute.resident(), f"{name} step {w}")
        sc.same_rows(on.sequential_rows(o.cells, o.q_hi, o.ref_ppm, o.alarm), got["rows"], f"{name} step {w} recurrence")
        sc.same_rows(o.results(w, G)["rows"], want["rows"][:G], f"{name} step {w} first G rows")
        seen.append(got)
    if c.check is not None:
        c.check(seen)


@pytest.mark.parametrize("B", [64, 128, 1024])
def test_the_scan_by_runs_equals_the_recurrence_on_random_series(B):
    rng = np.random.default_rng(B)
    for trial in range(6):
        n = rng.integers(0, 40, (4, B)).astype(np.uint64)
        b = np.minimum(n, rng.integers(0, 3 + trial, (4, B)).astype(np.uint64))
        n[rng.random((4, B)) < 0.5] = 0
        b = np.minimum(n, b)
        cells = (b << np.uint64(32)) | n
        q_hi = int(rng.integers(0, 1 << 40))
        for ref, alarm in ((20_000, 3), (250_000, 1), (999_999, 1), (1, 1_000_000)):
            a, s = on.scan_rows(cells, q_hi, ref, alarm), on.sequential_rows(cells, q_hi, ref, alarm)
            sc.same_rows(a, s, f"B={B} trial {trial} ref {ref}")
        # the operator itself, lane by lane as the device folds it: B / 64 bins a lane
        _n, _b, x = on._split(cells, q_hi, 250_000)
        per = B // 64
        for g in range(2):
            before, S = (0, 0), 0
            for lane in range(64):
                run = (0, 0)
                for t in range(lane * per, (lane + 1) * per):
                    run = on.combine(run, on.run_of(x[g, t]))
                    S = max(0, S + int(x[g, t]))
                    P = before[0] + run[0]
                    assert P - min(before[1], before[0] + run[1]) == S
                before = on.combine(before, run)
    assert on.combine((0, 0), (-4, -4)) == (-4, -4) and on.combine((3, 0), (-4, -4)) == (-1, -1)
    assert on.combine((-4, -4), (3, 0)) == (-1, -4)


def test_records_before_the_first_bins_and_a_first_cut_in_bin_zero():
    o = on.OnsetOracle(bins=64, bin_ns=sc.BIN, ref_ppm=250_000, alarm=1, span_cap=16, group_cap=1)
    assert o.q_hi == -1 and o.resident()["q_hi"] == -1
    recs = sc.timed([sc.BAD, sc.BAD], [0, 0], [1, sc.BIN - 1])
    r = o.results(o.step_records(recs, 5, 1), 1)["rows"][0]  # q_hi = 0: the ring covers bins -63 .. 0
    assert o.q_hi == 0 and int(r["onset_q"]) == 0 and int(r["alarm_q"]) == 0 and int(r["flags"]) == 0
    assert int(r["s_now"]) == 1_500_000 and int(r["state"]) == 2
    b = sc.Brute(bins=64, bin_ns=sc.BIN, ref_ppm=250_000, alarm=1, group_cap=1)
    sc.same_rows(b.step(recs, 5, 1)["rows"], o.results(0, 1)["rows"])


def test_every_configuration_check_and_every_refused_step():
    ok = dict(bins=1024, bin_ns=125_000_000, ref_ppm=20_000, alarm=3, span_cap=16384, group_cap=64, n_buffers=3,
              slo_ms=800.0)
    on.check_config(**ok)
    for key, lo, hi in (("bin_ns", 1_000_000, 60_000_000_000), ("ref_ppm", 1, 999_999), ("alarm", 1, 1_000_000),
                        ("group_cap", 1, 65536), ("n_buffers", 1, 64), ("ring_records_max", 1, (1 << 31) - 1)):
        small = dict(ok, bins=64)
        for good in (lo, hi):
            on.check_config(**dict(small, **{key: good}))
        for bad in (lo - 1, hi + 1):
            with pytest.raises(ValueError, match="breach onset"):
                on.check_config(**dict(small, **{key: bad}))
    for bins in (64, 128, 8192):
        on.check_config(**dict(ok, bins=bins))
    for bad in (dict(bins=32), dict(bins=16384), dict(bins=96), dict(bins=0), dict(span_cap=0), dict(slo_ms=float("nan")),
                dict(slo_ms=float("inf")), dict(slo_ms=-1.0), dict(group_cap=65536, bins=8192),
                dict(group_cap=32768, bins=8192), dict(span_cap=1 << 25)):
        with pytest.raises(ValueError, match="breach onset"):
            on.check_config(**dict(ok, **bad))
    on.check_config(**dict(ok, slo_ms=0.0, span_cap=1))
    on.check_config(**dict(ok, group_cap=32768, bins=4096))
    assert on.device_bytes(1024, 16384, 64) == 16384 * 64 + 64 * 1024 * 8 + (64 * 16 + 8) * 4
    with pytest.raises(ValueError, match="breach onset: bins"):
        on.OnsetOracle(bins=100)
    o = on.OnsetOracle(bins=64, bin_ns=sc.BIN, span_cap=4, group_cap=2, n_buffers=2)
    recs = sc.timed([1.0] * 5, [0] * 5, [sc.T0] * 5)
    cut = sc.T0 + 5
    with pytest.raises(ValueError, match="more spans than span_cap"):
        o.step_records(recs, cut, 1)
    for G in (3, -1):
        with pytest.raises(ValueError, match="n_groups out of range"):
            o.step_records(recs[:2], cut, G)
    for bad_cut in (0, -1):
        with pytest.raises(ValueError, match="cut_ns must be > 0"):
            o.step_records(recs[:2], bad_cut, 1)
    with pytest.raises(ValueError, match="whole 64-byte spans"):
        o.step([(recs.ctypes.data, 65)], cut, 1)
    assert o.n == 0 and o.q_hi == -1 and not o.cells.any() and not o.held, "a refused step changes nothing"
    for _ in range(3):
        o.step_records(recs[:2], cut, 1)
    with pytest.raises(IndexError, match="not held"):
        o.results(0, 1)
    assert int(o.results(2, 1)["rows"][0]["n_ring"]) == 6


def test_the_ring_bound_on_both_sides_and_expiry_frees_room():
    B = 64
    o = on.OnsetOracle(bins=B, bin_ns=sc.BIN, span_cap=64, group_cap=1, ring_records_max=100)
    q = sc.Q0

    def recs(n, at):
        return sc.timed([sc.GOOD] * n, [0] * n, [at * sc.BIN + 1] * n)

    o.step_records(recs(60, q), sc.cut_of(q), 1)
    o.step_records(recs(40, q + 10), sc.cut_of(q + 10), 1)   # exactly ring_records_max
    assert o.population_after(q + 10, 0) == 100
    before = (o.n, o.q_hi, o.cells.copy(), list(o.held))
    with pytest.raises(ValueError, match="ring_records_max"):
        o.step_records(recs(1, q + 10), sc.cut_of(q + 10), 1)
    with pytest.raises(ValueError, match="ring_records_max"):
        o.step_records(recs(1, q + B - 1), sc.cut_of(q + B - 1), 1)   # bin q is still in the ring
    assert (o.n, o.q_hi, list(o.held)) == (before[0], before[1], before[3]) and (o.cells == before[2]).all()
    o.step_records(np.zeros(0, sc.R.SPAN), sc.cut_of(q + 10), 1)      # an empty step is always taken
    with pytest.raises(ValueError, match="ring_records_max"):
        o.step_records(recs(61, q + B), sc.cut_of(q + B), 1)
    i = o.step_records(recs(60, q + B), sc.cut_of(q + B), 1)          # the first step's 60 are cleared: room again
    assert int(o.results(i, 1)["rows"][0]["n_ring"]) == 100 and len(o.held) == 2
    # spans offered count, observed or not: 30 skipped records fill the bound as well
    o = on.OnsetOracle(bins=B, bin_ns=sc.BIN, span_cap=64, group_cap=1, ring_records_max=30)
    o.step_records(sc.timed([1.0] * 30, [0] * 30, [q * sc.BIN] * 30, sc.R.SPAN_NO_SLI), sc.cut_of(q), 1)
    with pytest.raises(ValueError, match="ring_records_max"):
        o.step_records(recs(1, q), sc.cut_of(q), 1)


RESULT_KEYS = {"post", "conf", "feat", "pred", "evbits", "sli", "app", "late"}


def _pipeline_windows():
    rng = np.random.default_rng(7)
    G, B = 3, 64
    qs = [sc.Q0 + sc.PER_WINDOW * (w + 1) for w in range(6)]
    wins = [sc.edge_window(rng, 30, G, q, B) for q in qs]
    cuts = [sc.cut_of(q) for q in qs]
    cuts[3] = 0  # a cut without a time
    return wins, cuts, G, B


def test_pipeline_on_the_host_engine_carries_the_new_key_only_when_switched_on():
    from llm_slo_ebpf_toolkit_amd.pipeline.window import WindowPipeline

    wins, cuts, G, B = _pipeline_windows()
    off, none, _ = sc.run_pipeline("cpu", wins, cuts, G, 0)
    onr, ons, skipped = sc.run_pipeline("cpu", wins, cuts, G, B, onset_bin_ns=sc.BIN)
    ref = on.OnsetOracle(bins=B, bin_ns=sc.BIN, ref_ppm=250_000, alarm=3, span_cap=1024, group_cap=8, slo_ms=sc.SLO)
    assert none == [] and skipped == 1
    for w, (a, b, s) in enumerate(zip(off, onr, ons)):
        assert set(a) == RESULT_KEYS, "breach onset off: today's keys"
        assert set(b) == RESULT_KEYS | set(on.RESULT_KEYS)
        for key in RESULT_KEYS:
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"window {w} {key}")
        want = on.empty_result(G) if cuts[w] <= 0 else ref.results(ref.step_records(wins[w], cuts[w], G), G)
        sc.same_results(s, want, f"window {w}")
        sc.same_rows(b["onset_rows"], want["rows"], f"window {w}")
    assert any(int(r["onset_rows"]["state"].max()) == 2 for r in onr)
    assert (ons[3]["rows"]["onset_q"] == -1).all() and not ons[3]["rows"]["n_ring"].any()
    with pytest.raises(ValueError, match="one GPU: no communicator, no sharding"):
        WindowPipeline(1024, 64, 4, engine="cpu", shard=(0, 2), breach_onset=64)
    with pytest.raises(ValueError, match="breach onset: bins"):
        WindowPipeline(1024, 64, 4, engine="cpu", breach_onset=100)
    with pytest.raises(ValueError, match="breach onset: ref_ppm"):
        WindowPipeline(1024, 64, 4, engine="cpu", breach_onset=64, onset_ref_ppm=0)
    p = WindowPipeline(1024, 64, 4, engine="cpu", breach_onset=64, window_ms=2000.0)
    try:
        assert p.onset.bin_ns == 125_000_000, "a sixteenth of the window by default"
    finally:
        p.close()


# ---- the agent ----------------------------------------------------------------------------------------

def _agent(tmp_path, tag, **kw):
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions

    log = tmp_path / f"decisions-{tag}.jsonl"
    o = AgentOptions(engine="cpu", source="replay", gpus=1, window_events=2048, window_spans=128, window_groups=8,
                     window_ms=300, metrics_bind="", output="stdout", ring_name=f"/mislo-on-{tag}-{os.getpid()}",
                     config="", min_confidence=0.0, scenario="full", disable_overhead_guard=True,
                     decision_log=str(log), **kw)
    out = io.StringIO()
    a = Agent(o, out_stream=out)
    seen = []
    inner = a._attributions

    def spy(G, names, res, t_ns, model):
        attrs = inner(G, names, res, t_ns, model)
        seen.append((res, attrs, t_ns))
        return attrs

    a._attributions = spy
    try:
        assert a.run_windows(max_windows=4) == 0
    finally:
        a.close()
    return a, seen, [json.loads(ln) for ln in log.read_text().splitlines()], out.getvalue()


def test_agent_flags_defaults_and_the_one_gpu_rule():
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions
    from llm_slo_ebpf_toolkit_amd.cli.agent import parse

    o, _ = parse(["--engine", "cpu", "--breach-onset", "--onset-bin-ms", "50", "--onset-bins", "256", "--onset-ref-burn",
                  "1.5", "--onset-alarm-breaches", "5"])
    assert (o.breach_onset, o.onset_bin_ms, o.onset_bins, o.onset_ref_burn, o.onset_alarm_breaches) == (True, 50.0, 256, 1.5, 5)
    d = parse([])[0]
    assert (d.breach_onset, d.onset_bin_ms, d.onset_bins, d.onset_ref_burn, d.onset_alarm_breaches) == (False, 0.0, 1024, 2.0, 3)
    assert AgentOptions().breach_onset is False
    kw = dict(engine="cpu", source="replay", config="", output="stdout", metrics_bind="")
    a = Agent(AgentOptions(ring_name=f"/mislo-on2-{os.getpid()}", window_ms=2000, slo_target=0.99, **kw))
    try:
        assert a.onset_bin_ns() == 125_000_000 and a.onset_ref_ppm() == 20_000  # window / 16; 2.0 x the 1 % budget
    finally:
        a.close()
    a = Agent(AgentOptions(ring_name=f"/mislo-on3-{os.getpid()}", window_ms=8, onset_ref_burn=500.0, **kw))
    try:
        assert a.onset_bin_ns() == 1_000_000 and a.onset_ref_ppm() == 999_999  # at least 1 ms; clamped
    finally:
        a.close()
    assert on.ref_ppm_of(0.0, 0.99) == 1 and on.ref_ppm_of(2.0, 0.999) == 2000
    a = Agent(AgentOptions(gpus=2, ring_name=f"/mislo-on4-{os.getpid()}", breach_onset=True, **kw))
    try:
        with pytest.raises(ValueError, match="--breach-onset runs on one GPU"):
            a.run_windows(max_windows=1)
    finally:
        a.close()


def test_the_decision_log_entry_and_the_series_from_a_fabricated_result():
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions
    from llm_slo_ebpf_toolkit_amd.agent.metrics import AgentMetrics
    from llm_slo_ebpf_toolkit_amd.export.prometheus import parse_exposition

    rows = on.quiet_rows(3)
    rows[1] = (2, 0, 1000, 1004, 3_250_000, 4_000_000, 9, 5, 40, 6, (0, 0))
    rows[2] = (1, 1, 937, -1, 500_000, 500_000, 2, 1, 2, 1, (0, 0))
    rows[0]["n_ring"] = 7
    res = {"onset_rows": rows}
    a = Agent(AgentOptions(engine="cpu", source="replay", config="", output="stdout", metrics_bind="", window_ms=160,
                           ring_name=f"/mislo-on5-{os.getpid()}", breach_onset=True))
    try:
        bin_ns = a.onset_bin_ns()
        assert bin_ns == 10_000_000
        cut = 1010 * bin_ns + 5_000_000
        keys = {"state", "onset_ts_ns", "alarm_ts_ns", "age_ms", "delay_ms", "excess", "requests", "breaches", "clipped"}
        e = [a._onset_entry(res, g, cut) for g in range(3)]
        assert all(set(x) == keys for x in e)
        assert e[0] == {"state": 0, "onset_ts_ns": None, "alarm_ts_ns": None, "age_ms": None, "delay_ms": None,
                        "excess": 0.0, "requests": 0, "breaches": 0, "clipped": False}
        assert e[1] == {"state": 2, "onset_ts_ns": 1000 * bin_ns, "alarm_ts_ns": 1004 * bin_ns, "age_ms": 105.0,
                        "delay_ms": 40.0, "excess": 3.25, "requests": 9, "breaches": 5, "clipped": False}
        assert e[2]["state"] == 1 and e[2]["clipped"] is True and e[2]["delay_ms"] is None and e[2]["alarm_ts_ns"] is None
        assert e[2]["age_ms"] == 735.0 and e[2]["excess"] == 0.5
        json.dumps(e)
    finally:
        a.close()
    m = AgentMetrics("probe", "auto", [], [])
    stats = {"observed": 50, "invalid": 1, "out_of_group": 2, "no_time": 3, "future": 4, "too_old": 5}
    m.observe_onset(res, stats, ["rag", "chat"], cut, bin_ns)
    m.observe_onset(res, stats, ["rag", "chat"], cut, bin_ns)
    v = parse_exposition(m.registry.exposition())
    assert v['llm_slo_agent_breach_onset_age_seconds{service="rag"}'] == 0
    assert v['llm_slo_agent_breach_onset_age_seconds{service="chat"}'] == pytest.approx(0.105)
    assert v['llm_slo_agent_breach_onset_age_seconds{service="group-2"}'] == pytest.approx(0.735)
    assert [v[f'llm_slo_agent_breach_onset_state{{service="{s}"}}'] for s in ("rag", "chat", "group-2")] == [0, 2, 1]
    for reason in on.EVENT_STATS:
        assert v[f'llm_slo_agent_breach_onset_events_total{{reason="{reason}"}}'] == 2 * stats[reason]


@pytest.mark.timeout(120)
def test_the_agent_logs_an_onset_per_scored_group_and_off_means_nothing_new(tmp_path):
    from llm_slo_ebpf_toolkit_amd.contracts import validator

    a, seen, rows, out = _agent(tmp_path, "on", breach_onset=True, onset_bins=256)
    assert seen and all("onset_rows" in res for res, _, _ in seen)
    assert rows and all("onset" in r for r in rows)
    bin_ns = a.onset_bin_ns()
    for res, _, t_ns in seen:
        for r in (r for r in rows if r["t_ns"] == int(t_ns)):
            row, e = res["onset_rows"][r["group"]], r["onset"]
            assert e["state"] == int(row["state"]) and e["requests"] == int(row["n_exc"]) and e["breaches"] == int(row["b_exc"])
            if e["state"]:
                assert e["onset_ts_ns"] == int(row["onset_q"]) * bin_ns <= t_ns and e["age_ms"] >= 0
    assert any(r["onset"]["state"] for r in rows), "the replay's breaching groups open an excursion"
    emitted = [json.loads(ln) for ln in out.splitlines() if ln.startswith('{"incident_id"')]
    assert emitted
    for d in emitted:
        assert "onset" not in d
        validator.validate("incident-attribution", d)
    assert 'llm_slo_agent_breach_onset_state{service="' in a.metrics.registry.exposition()
    b, seen_off, rows_off, out_off = _agent(tmp_path, "off")
    assert seen_off and all("onset_rows" not in res for res, _, _ in seen_off) and all("onset" not in r for r in rows_off)
    assert "llm_slo_agent_breach_onset_state{" not in b.metrics.registry.exposition()
    # the replay is cut by the wall clock, so two runs need not see the same windows: the shapes are compared
    off = [json.loads(ln) for ln in out_off.splitlines() if ln.startswith('{"incident_id"')]
    assert off and {frozenset(d) for d in off} == {frozenset(d) for d in emitted}, "emitted incidents keep their fields"
    assert {frozenset(r) | {"onset"} for r in rows_off} == {frozenset(r) for r in rows}


# ---- the tracker's host side under the host sanitizers ------------------------------------------------

HOST_KEYS = [(0, 0), (0, 1), (1, 0), (63, 1023), (65535, 8191), (7, 4242)]
HOST_TIMES = [(1, 1_000_000), (999_999, 1_000_000), (1_000_000, 1_000_000), (1_700_000_000_123_456_789, 125_000_000),
              (1_700_000_000_123_456_789, 60_000_000_000), (59_999_999_999, 60_000_000_000)]


@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="needs g++")
@pytest.mark.timeout(300)
def test_onset_host_side_under_address_and_ub_sanitizers(tmp_path):
    """ops/csrc/onset_host.h (bin rule, slot, scan operator, row, argument checks, layout, ring bound) needs
    no device: a stand-alone program over it, built with AddressSanitizer + UBSan, run as a child process.
    It prints lds_hash for HOST_KEYS and bin_of / slot_of for HOST_TIMES, which must be the Python mirror's."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "llm_slo_ebpf_toolkit_amd", "ops", "csrc")
    exe = tmp_path / "onset_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-Wall", "-Werror", f"-I{csrc}", os.path.join(root, "tests", "native", "onset_host_check.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "onset host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
    got = [tuple(int(x) for x in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("lds_hash ")]
    assert got == [(g, s, on.lds_hash(on.lds_key(g, s))) for g, s in HOST_KEYS]
    assert all(0 <= h < 256 for _, _, h in got)
    got = [tuple(int(x) for x in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("bin_of ")]
    assert got == [(t, b, on.bin_of(t, b), on.slot_of(on.bin_of(t, b), 1024)) for t, b in HOST_TIMES]
