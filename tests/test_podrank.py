"""The per-pod breach breakdown's rules on the host (pipeline/podrank.py): the numpy oracle against a
brute-force dict of dicts, the ranking key, the horizon, the capacity's two sides, every refusal, the
host engine's result keys, the agent's decision-log entry and series, and the tracker's host side
(ops/csrc/podrank_host.h) under the host sanitizers. The device tracker against the oracle:
tests/test_podrank_gpu.py."""

import io
import json
import os

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.pipeline import podrank as pr
from tests import podrank_scenarios as sc

F32 = np.float32


def _drive(oracle, wins, groups, K, H, C, what=""):
    """Every window through the oracle and the brute force; every result and the lists equal."""
    tots, pairs = [], []
    for w, (recs, G) in enumerate(zip(wins, groups)):
        t, p, stats = sc.brute_pairs(recs, G)
        tots.append(t), pairs.append(p)
        i = oracle.step_records(recs, G)
        assert not oracle.overflowed(i)
        want = sc.brute_results(tots, pairs, stats, C, K, H)
        sc.same_results(oracle.results(i, C), want, f"{what} window {w}")
        held = oracle.resident()
        for age in range(min(H, w + 1)):
            got = pr.sort_pairs(held[(w - age) % H])
            assert got.tobytes() == sc.pairs_array(pairs[w - age]).tobytes(), (what, w, age)
    return tots, pairs


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("H", [1, 3])
def test_oracle_equals_a_brute_force_dict_of_dicts_for_both_scopes(K, H):
    rng = np.random.default_rng(100 * K + H)
    G, C = 3, 5
    wins = [sc.edge_window(rng, int(n), G) for n in rng.integers(0, 80, 6)]
    _drive(pr.PodRankOracle(k=K, windows=H, pair_cap=256, span_cap=1024, group_cap=C), wins, [G] * len(wins), K, H, C)


def test_edge_values_count_and_breach_where_the_rule_says():
    o = pr.PodRankOracle(k=8, windows=1, pair_cap=64, span_cap=256, group_cap=2, slo_ms=800.0)
    above = np.nextafter(F32(800), F32(np.inf))
    ttft = [F32(800.0), above, F32(np.inf), F32(-0.0), F32(np.nan), F32(-1.0), F32(100.0), F32(900.0), F32(900.0),
            F32(900.0), F32(50.0)]
    pods = [1, 2, 3, 4, 5, 6, 0, (1 << 20) - 1, 1 << 20, 9, 9]
    grp = [0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0]  # group 2 = n_groups: out of group
    r = o.results(o.step_records(sc.pod_spans(ttft, grp, pods), 2), 2)
    st = pr.stats_dict(r["stats"])
    assert st == {"observed": 8, "invalid": 2, "out_of_group": 1, "pod_out_of_range": 1, "pair_overflow": 0}
    assert r["win_n"].tolist() == [8, 0] and r["win_b"].tolist() == [4, 0]  # above, +inf, the two 900s of group 0
    assert r["win_pods"].tolist() == [7, 0] and r["win_pods_b"].tolist() == [3, 0]  # pod 2^20 has no row
    top = r["win_top"][0][:int(r["win_k_top"][0])]
    assert top["pod_id"].tolist() == [2, 3, (1 << 20) - 1]  # one breach, one request each: the lower pod first
    assert np.isposinf(top["max_ttft"][1]) and int(top["sum_milli"][1]) == 2 ** 21 * 1000  # +inf: a breach, clamped sum
    assert top["max_ttft"][0] == above and int(top["sum_milli"][0]) == 800000  # rint(800.00006 * 1000)
    # -0.0 is counted, ranks as +0.0; pod 0 is an ordinary pod; equal to the SLO is no breach
    rows = {int(p["pod"]): p for p in o.resident()[0]}
    assert set(rows) == {0, 1, 2, 3, 4, 9, (1 << 20) - 1}
    assert int(rows[4]["max_bits"]) == 0 and int(rows[4]["n"]) == 1 and int(rows[1]["b"]) == 0 and int(rows[0]["n"]) == 1


def test_the_three_tie_levels_of_the_ranking_key():
    # pod: (requests, breaches). More breaches first; then fewer requests; then the lower pod id.
    spec = {10: (5, 3), 11: (4, 3), 12: (4, 3), 13: (9, 4), 14: (2, 1), 15: (3, 0)}
    ttft, pods = [], []
    for pod, (n, b) in spec.items():
        ttft += [900.0] * b + [100.0] * (n - b)
        pods += [pod] * n
    rng = np.random.default_rng(3)
    order = rng.permutation(len(ttft))
    o = pr.PodRankOracle(k=8, windows=1, pair_cap=16, span_cap=64, group_cap=1)
    r = o.results(o.step_records(sc.pod_spans(np.array(ttft)[order], [0] * len(ttft), np.array(pods)[order]), 1), 1)
    assert int(r["win_k_top"][0]) == 5 and int(r["win_pods"][0]) == 6 and int(r["win_pods_b"][0]) == 5
    assert r["win_top"][0]["pod_id"][:5].tolist() == [13, 11, 12, 10, 14]
    assert not r["win_top"][0][5:].view(np.uint8).any(), "rows past k_top are all zero"
    # the key: order, round trip, uniqueness, never 0
    b = np.array([1, 1, 1, 2, (1 << 22) - 1], np.uint64)
    n = np.array([1, 1, 2, (1 << 22) - 1, (1 << 22) - 1], np.uint64)
    pod = np.array([0, (1 << 20) - 1, 0, 5, (1 << 20) - 1], np.uint64)
    key = pr.rank_key(b, n, pod)
    assert key.dtype == np.uint64 and (key > 0).all() and len(set(key.tolist())) == len(key)
    assert key[0] > key[1] > key[2] and key[3] > key[0] and key[4] > key[3]
    for got, want in zip(pr.rank_unpack(key), (b, n, pod)):
        np.testing.assert_array_equal(got, want)
    rng = np.random.default_rng(5)
    b, n, pod = rng.integers(1, 1 << 22, 500), rng.integers(1, 1 << 22, 500), rng.integers(0, 1 << 20, 500)
    key = pr.rank_key(b, n, pod)
    by_key = np.argsort(key)[::-1]
    by_rule = np.lexsort((pod, n, -b))
    np.testing.assert_array_equal(by_key, by_rule)


def test_horizon_wraps_with_an_empty_step_and_a_step_without_groups_and_a_pod_ages_out_after_h_steps():
    K, H, C = 3, 3, 4
    rng = np.random.default_rng(11)
    o = pr.PodRankOracle(k=K, windows=H, pair_cap=64, span_cap=512, group_cap=C)
    lone = sc.pod_spans([950.0, 20.0], [1, 1], [77, 77])  # pod 77 of group 1: step 0 only
    wins = [lone, sc.edge_window(rng, 30, 3), np.zeros(0, sc.R.SPAN), sc.edge_window(rng, 20, 2),
            sc.edge_window(rng, 25, 3), sc.edge_window(rng, 10, 4), sc.edge_window(rng, 30, 3)]
    groups = [2, 3, 3, 0, 3, 4, 3]
    _drive(o, wins, groups, K, H, C, "wrap")
    # the lone pod: in `recent` for steps 0 .. H-1, gone at step H
    o = pr.PodRankOracle(k=K, windows=H, pair_cap=64, span_cap=512, group_cap=C)
    for step in range(H + 1):
        r = o.results(o.step_records(lone if step == 0 else np.zeros(0, sc.R.SPAN), 2 if step != 2 else 0), C)
        here = step < H
        assert int(r["rec_pods"][1]) == int(here) and int(r["rec_k_top"][1]) == int(here), step
        assert int(r["rec_n"][1]) == 2 * here and int(r["rec_b"][1]) == int(here), step
        assert int(r["win_n"][1]) == (2 if step == 0 else 0)
        if here:
            assert int(r["rec_top"][1][0]["pod_id"]) == 77


@pytest.mark.parametrize("n_hot", [2, 3, 7])
def test_fewer_and_more_breaching_pods_than_k(n_hot):
    K = 3
    ttft, pods = [], []
    for pod in range(1, 10):  # pod p breaches p times when hot
        ttft += ([900.0] * pod if pod <= n_hot else []) + [10.0]
        pods += [pod] * ((pod if pod <= n_hot else 0) + 1)
    o = pr.PodRankOracle(k=K, windows=2, pair_cap=32, span_cap=128, group_cap=2)
    r = o.results(o.step_records(sc.pod_spans(ttft, [1] * len(ttft), pods), 2), 2)
    assert int(r["win_pods"][1]) == 9 and int(r["win_pods_b"][1]) == n_hot and int(r["win_k_top"][1]) == min(K, n_hot)
    want = list(range(n_hot, 0, -1))[:K]
    assert r["win_top"][1]["pod_id"][:len(want)].tolist() == want
    assert not r["win_top"][1][len(want):].view(np.uint8).any() and not r["win_top"][0].view(np.uint8).any()
    sc.same_rows(r["win_top"], r["rec_top"])


def test_the_capacity_holds_exactly_pair_cap_pairs_and_beyond_it_keeps_the_totals_exact():
    cap = 8
    pods = list(range(1, cap + 1))
    recs = sc.pod_spans([900.0, 10.0] * cap, [0] * (2 * cap), np.repeat(pods, 2))
    o = pr.PodRankOracle(k=3, windows=2, pair_cap=cap, span_cap=128, group_cap=1)
    i = o.step_records(recs, 1)
    assert not o.overflowed(i) and pr.stats_dict(o.results(i, 1)["stats"])["pair_overflow"] == 0
    t, p, stats = sc.brute_pairs(recs, 1)
    sc.same_results(o.results(i, 1), sc.brute_results([t], [p], stats, 1, 3, 2))
    more = sc.pod_spans([900.0, 10.0] * (cap + 5), [0] * (2 * cap + 10), np.repeat(list(range(1, cap + 6)), 2))
    i = o.step_records(more, 1)
    assert o.overflowed(i)
    r = o.results(i, 1)
    t, p, _ = sc.brute_pairs(more, 1)
    sc.overflow_invariants(r, p, t, o.resident()[i % 2], cap)
    assert pr.stats_dict(r["stats"])["pair_overflow"] == 10 and int(r["win_pods"][0]) == cap
    assert int(r["rec_n"][0]) == 2 * cap + 2 * (cap + 5), "the horizon's totals do not depend on the pair table"


def test_slot_hash_and_table_sizes():
    assert pr.fmix64(0) == 0 and pr.fmix64(1) == 0xB456BCFC34C2CB2C  # murmur3's finalizer
    assert pr.pair_key(0, 0) == 1 << 32 and pr.pair_key(65535, (1 << 20) - 1) == (65536 << 32) | 0xFFFFF
    assert pr.window_slots(8) == 16 and pr.window_slots(4096) == 8192 and pr.window_slots(5) == 16
    assert pr.window_slots(1) == 2 and pr.recent_slots(4096, 3) == 32768
    pods = sc.colliding_pods(0, 16, 15, 8)
    assert len(set(pods)) == 8 and all(pr.slot_of(0, p, 16) == 15 for p in pods)
    assert all(0 <= pr.slot_of(g, p, 1 << 13) < 1 << 13 for g in range(4) for p in range(50))


def test_every_configuration_check_and_every_refused_step():
    ok = dict(k=3, windows=3, pair_cap=4096, span_cap=16384, group_cap=64, n_buffers=3, slo_ms=800.0)
    pr.check_config(**ok)
    for key, lo, hi in (("k", 1, 8), ("windows", 1, 16), ("pair_cap", 1, 1 << 20), ("group_cap", 1, 65536),
                        ("n_buffers", 1, 64)):
        small = dict(ok, span_cap=64, pair_cap=64)  # both ends fit the 2 GiB and the count bound
        small[key] = lo
        pr.check_config(**small)
        small[key] = hi
        pr.check_config(**small)
        for bad in (lo - 1, hi + 1):
            with pytest.raises(ValueError, match="pod breakdown"):
                pr.check_config(**dict(small, **{key: bad}))
    pr.check_config(**dict(ok, span_cap=1))
    pr.check_config(**dict(ok, span_cap=(1 << 22) // 3, windows=3))   # 1398101 * 3 < 2^22
    for bad in (dict(span_cap=0), dict(span_cap=(1 << 22) // 3 + 1, windows=3), dict(span_cap=1 << 18, windows=16),
                dict(slo_ms=float("nan")), dict(slo_ms=float("inf")), dict(slo_ms=-1.0)):
        with pytest.raises(ValueError, match="pod breakdown"):
            pr.check_config(**dict(ok, **bad))
    pr.check_config(**dict(ok, slo_ms=0.0))
    # the 2 GiB bound guards the other bounds: the largest tables they allow stay below it
    assert pr.device_bytes(8, 16, 1 << 20, (1 << 18) - 1, 65536) < 1 << 31
    assert pr.device_bytes(3, 3, 4096, 16384, 64) == 16384 * 64 + (8192 + 32768 + 3 * 4096) * 28 + 8 * 64 * 4 \
        + 2 * 64 * 3 * 8 + pr.layout_words(64, 3) * 4 + 16
    with pytest.raises(ValueError, match="pod breakdown: k"):
        pr.PodRankOracle(k=0)
    o = pr.PodRankOracle(k=2, windows=2, pair_cap=16, span_cap=4, group_cap=2, n_buffers=2)
    recs = sc.pod_spans([1.0] * 5, [0] * 5, [1] * 5)
    with pytest.raises(ValueError, match="more spans than span_cap"):
        o.step_records(recs, 1)
    with pytest.raises(ValueError, match="n_groups out of range"):
        o.step_records(recs[:2], 3)
    with pytest.raises(ValueError, match="n_groups out of range"):
        o.step_records(recs[:2], -1)
    with pytest.raises(ValueError, match="whole 64-byte spans"):
        o.step([(recs.ctypes.data, 65)], 1)
    assert o.n == 0, "a refused step changes nothing"
    for _ in range(3):
        o.step_records(recs[:2], 1)
    with pytest.raises(IndexError, match="not held"):
        o.results(0, 1)
    assert int(o.results(2, 1)["win_n"][0]) == 2


RESULT_KEYS = {"post", "conf", "feat", "pred", "evbits", "sli", "app", "late"}


def test_pipeline_on_the_host_engine_carries_the_new_keys_only_when_switched_on():
    from llm_slo_ebpf_toolkit_amd.pipeline.window import WindowPipeline

    rng = np.random.default_rng(7)
    G, K = 3, 3
    wins = [sc.edge_window(rng, int(n), G) for n in rng.integers(0, 40, 6)]
    off, none = sc.run_pipeline("cpu", wins, G, 0)
    on, pods = sc.run_pipeline("cpu", wins, G, K)
    ref = pr.PodRankOracle(k=K, windows=3, pair_cap=256, span_cap=1024, group_cap=8, slo_ms=sc.SLO)
    assert none == []
    for w, (a, b, s) in enumerate(zip(off, on, pods)):
        assert set(a) == RESULT_KEYS, "pod breakdown off: today's keys"
        assert set(b) == RESULT_KEYS | set(pr.RESULT_KEYS)
        for key in RESULT_KEYS:
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"window {w} {key}")
        want = ref.results(ref.step_records(wins[w], G), G)
        sc.same_results(s, want, f"window {w}")
        keyed = pr.result_keys(want)
        for key in pr.RESULT_KEYS:
            if key in ("pod_win_top", "pod_rec_top"):
                sc.same_rows(b[key], keyed[key], f"window {w} {key}")
            else:
                np.testing.assert_array_equal(b[key], keyed[key], err_msg=f"window {w} {key}")
    assert sum(int(r["pod_win_b"].sum()) for r in on) > 10
    with pytest.raises(ValueError, match="one GPU: no communicator, no sharding"):
        WindowPipeline(1024, 64, 4, engine="cpu", shard=(0, 2), pod_breakdown=3)
    with pytest.raises(ValueError, match="pod breakdown: k"):
        WindowPipeline(1024, 64, 4, engine="cpu", pod_breakdown=9)
    with pytest.raises(ValueError, match="pod breakdown: pair_cap"):
        WindowPipeline(1024, 64, 4, engine="cpu", pod_breakdown=3, pod_pairs=0)


# ---- the agent ----------------------------------------------------------------------------------------

def _agent(tmp_path, tag, **kw):
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions

    log = tmp_path / f"decisions-{tag}.jsonl"
    o = AgentOptions(engine="cpu", source="replay", gpus=1, window_events=2048, window_spans=128, window_groups=8,
                     window_ms=300, metrics_bind="", output="stdout", ring_name=f"/mislo-pr-{tag}-{os.getpid()}",
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

    o, _ = parse(["--engine", "cpu", "--pod-breakdown", "5", "--pod-breakdown-windows", "2", "--pod-pairs", "512"])
    assert (o.pod_breakdown, o.pod_breakdown_windows, o.pod_pairs) == (5, 2, 512)
    d = parse([])[0]
    assert (d.pod_breakdown, d.pod_breakdown_windows, d.pod_pairs) == (0, 3, 4096) and AgentOptions().pod_breakdown == 0
    a = Agent(AgentOptions(engine="cpu", source="replay", config="", output="stdout", metrics_bind="", gpus=2,
                           ring_name=f"/mislo-pr2-{os.getpid()}", pod_breakdown=3))
    try:
        with pytest.raises(ValueError, match="--pod-breakdown runs on one GPU"):
            a.run_windows(max_windows=1)
    finally:
        a.close()


@pytest.mark.timeout(120)
def test_the_decision_log_lists_the_recent_pods_worst_first_and_the_series_follow(tmp_path):
    from llm_slo_ebpf_toolkit_amd.contracts import validator
    from llm_slo_ebpf_toolkit_amd.export.prometheus import parse_exposition

    a, seen, rows, out = _agent(tmp_path, "on", pod_breakdown=3, pod_breakdown_windows=3)
    assert seen and all(set(pr.RESULT_KEYS) <= set(res) for res, _ in seen)
    assert rows and all("pods" in r for r in rows)
    fields = {"pod", "pod_id", "requests", "breaches", "share", "ttft_mean_ms", "ttft_max_ms"}
    names = a.pod_ids.names()
    busy = [r for r in rows if r["pods"]["top"]]
    assert busy, "a window whose group breaches ranks its pods"
    for r in rows:
        p = r["pods"]
        assert set(p) == {"seen", "breaching", "requests", "breaches", "top"}
        assert p["seen"] >= p["breaching"] >= len(p["top"]) and len(p["top"]) == min(3, p["breaching"])
        assert all(set(e) == fields for e in p["top"])
        order = [(-e["breaches"], e["requests"], e["pod_id"]) for e in p["top"]]
        assert order == sorted(order), "worst first"
        for e in p["top"]:
            assert 1 <= e["breaches"] <= e["requests"] <= p["requests"]
            assert e["share"] == pytest.approx(e["breaches"] / p["breaches"], abs=1e-4)
            assert e["pod"] == ((names[e["pod_id"]] or "") if e["pod_id"] < len(names) else "")
            assert 0 <= e["ttft_mean_ms"] <= e["ttft_max_ms"] + 1e-3
    # the recent scope of the log's last window of a group against the results the agent saw
    res, _ = seen[-1]
    last = {r["group"]: r for r in rows if r["t_ns"] == rows[-1]["t_ns"]}
    assert last
    for g, r in last.items():
        assert r["pods"]["seen"] == int(res["pod_rec_pods"][g]) and r["pods"]["breaches"] == int(res["pod_rec_b"][g])
    # incidents stay as they are: the contract is closed
    emitted = [json.loads(ln) for ln in out.splitlines() if ln.startswith('{"incident_id"')]
    assert emitted
    for d in emitted:
        assert "pods" not in d
        validator.validate("incident-attribution", d)
    m = parse_exposition(a.metrics.registry.exposition())
    for g in range(len(res["pod_rec_n"])):
        svc = f'{{service="svc-{g + 1}"}}'
        assert m["llm_slo_agent_pods_seen" + svc] == int(res["pod_rec_pods"][g])
        assert m["llm_slo_agent_pods_breaching" + svc] == int(res["pod_rec_pods_b"][g])
        b = int(res["pod_rec_b"][g])
        share = int(res["pod_rec_top"][g][0]["b"]) / b if b else 0.0
        assert m["llm_slo_agent_breach_top_pod_share" + svc] == pytest.approx(share)
    for reason in pr.EVENT_STATS:
        assert m[f'llm_slo_agent_pod_breakdown_events_total{{reason="{reason}"}}'] == 0
    # no per-pod label series: the new series are labelled by service or reason alone
    new = [ln for ln in a.metrics.registry.exposition().splitlines()
           if ln.startswith(("llm_slo_agent_pods_", "llm_slo_agent_breach_top_pod_share", "llm_slo_agent_pod_breakdown_"))]
    assert new and not any("pod=" in ln or "pod_id=" in ln for ln in new)


@pytest.mark.timeout(120)
def test_with_the_flag_off_nothing_new_appears(tmp_path):
    a, seen, rows, out = _agent(tmp_path, "off")
    assert seen and all(not set(pr.RESULT_KEYS) & set(res) for res, _ in seen)
    assert rows and all("pods" not in r for r in rows)
    assert "llm_slo_agent_pods_seen{" not in a.metrics.registry.exposition()
    _b, _seen, rows_on, out_on = _agent(tmp_path, "on2", pod_breakdown=2)
    emitted = [json.loads(ln) for ln in out.splitlines() if ln.startswith('{"incident_id"')]
    on = [json.loads(ln) for ln in out_on.splitlines() if ln.startswith('{"incident_id"')]

    def plain(d, drop=()):
        return {k: v for k, v in d.items() if k not in drop and k not in ("incident_id", "timestamp", "t_ns")}

    assert len(on) == len(emitted) and len(rows_on) == len(rows)
    assert [plain(x) for x in emitted] == [plain(y) for y in on], "emitted incidents do not change"
    assert [plain(x) for x in rows] == [plain(y, ("pods",)) for y in rows_on]


def test_pod_metrics():
    from llm_slo_ebpf_toolkit_amd.agent.metrics import AgentMetrics
    from llm_slo_ebpf_toolkit_amd.export.prometheus import parse_exposition

    o = pr.PodRankOracle(k=2, windows=2, pair_cap=2, span_cap=64, group_cap=2)
    m = AgentMetrics("probe", "auto", [], [])
    steps = ((([900.0, 900.0, 900.0, 40.0, float("nan")], [0, 0, 0, 0, 0], [1, 1, 2, 3, 1]), 2),  # pod 3 overflows
             (([60.0, 75.0, 30.0], [1, 5, 0], [1 << 20, 1, 4]), 2))
    for (vals, grp, pods), G in steps:
        r = o.results(o.step_records(sc.pod_spans(vals, grp, pods), G), G)
        m.observe_pods(pr.result_keys(r), pr.stats_dict(r["stats"]), ["rag"])
    v = parse_exposition(m.registry.exposition())
    assert v['llm_slo_agent_pods_seen{service="rag"}'] == 3  # pods 1, 2 of the first window, 4 of the second
    assert v['llm_slo_agent_pods_breaching{service="rag"}'] == 2
    assert v['llm_slo_agent_breach_top_pod_share{service="rag"}'] == pytest.approx(2 / 3)
    assert v['llm_slo_agent_pods_seen{service="group-1"}'] == 0  # its one record's pod has no row
    assert v['llm_slo_agent_breach_top_pod_share{service="group-1"}'] == 0
    want = {"invalid": 1, "out_of_group": 1, "pod_out_of_range": 1, "pair_overflow": 1}
    for reason, n in want.items():
        assert v[f'llm_slo_agent_pod_breakdown_events_total{{reason="{reason}"}}'] == n


# ---- the tracker's host side under the host sanitizers ------------------------------------------------

HOST_SLOTS = [(0, 0, 2), (0, 1, 16), (0, 5, 16), (3, 77, 8192), (63, (1 << 20) - 1, 32768), (65535, 12345, 1 << 21),
              (1, 0xFFFFF, 16), (7, 7, 1 << 25)]


@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="needs g++")
@pytest.mark.timeout(300)
def test_podrank_host_side_under_address_and_ub_sanitizers(tmp_path):
    """ops/csrc/podrank_host.h (keys, slot hash, row, argument checks, result layout) needs no device:
    a stand-alone program over it, built with AddressSanitizer + UBSan, run as a child process. It
    prints slot_of for HOST_SLOTS, which must be the Python mirror's."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "llm_slo_ebpf_toolkit_amd", "ops", "csrc")
    exe = tmp_path / "podrank_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-Wall", "-Werror", f"-I{csrc}", os.path.join(root, "tests", "native", "podrank_host_check.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "podrank host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
    got = [tuple(int(x) for x in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("slot_of ")]
    assert got == [(g, pod, slots, pr.slot_of(g, pod, slots)) for g, pod, slots in HOST_SLOTS]
