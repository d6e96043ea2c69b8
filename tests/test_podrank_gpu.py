"""The pod-breakdown tracker on the device (ops/csrc/podrank.hip) against the host implementation
(pipeline/podrank.py): the same windows through both, step by step -- every result array and the
sorted resident lists must be equal, rows compared as bytes. Small windows with the rule's edge
values, horizons that wrap, one hot pair and one wide group with the LDS table on and off, pairs that
all collide on the table's last slot, the capacity's two sides, records split over ranges, a group
count that changes, a randomised run, and the whole way through WindowPipeline and the rings against
the host engine."""

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.pipeline import podrank as pr
from tests import podrank_scenarios as sc

pytestmark = pytest.mark.gpu


def _pair(k, windows, group_cap, span_cap=1024, pair_cap=256, lds=True, **kw):
    from llm_slo_ebpf_toolkit_amd.ops.podrank import PodRankTracker

    kw = dict(k=k, windows=windows, span_cap=span_cap, group_cap=group_cap, pair_cap=pair_cap, slo_ms=sc.SLO, **kw)
    return PodRankTracker(lds=lds, **kw), pr.PodRankOracle(**kw)


def _equal_step(dev, ref, recs, G, what, ranges=None):
    i = dev.step_records(recs, G) if ranges is None else dev.step(ranges, G)
    assert i == ref.step_records(recs, G)
    assert not ref.overflowed(i), what
    # every row of group_cap: a group absent from the step still ages
    a, b = dev.results(i, dev.group_cap), ref.results(i, ref.group_cap)
    sc.same_results(a, b, what)
    sc.same_results(dev.results(i, G), ref.results(i, G), what)
    sc.same_resident(dev.resident(), ref.resident(), what)
    return a


def _run(dev, ref, wins, groups):
    total = np.zeros(pr.N_STATS, np.int64)
    try:
        for w, (recs, G) in enumerate(zip(wins, groups)):
            total += _equal_step(dev, ref, recs, G, f"step {w}")["stats"].astype(np.int64)
    finally:
        dev.close()
    return pr.stats_dict(total)


@pytest.mark.parametrize("K", [1, 3, 8])
def test_small_windows_with_the_edge_values_equal_the_oracle_after_every_step(K):
    rng = np.random.default_rng(17 + K)
    G = 3
    wins = [sc.edge_window(rng, 40, G) for _ in range(8)]
    tot = _run(*_pair(K, 3, G), wins, [G] * 8)
    n_edge, n_pods = len(sc.EDGE_TTFT), len(sc.EDGE_PODS)
    # per window: 40 + per group the edge values (2 of them invalid) and two records of every edge pod
    # (2 of the pods out of range); 4 records out of group
    assert tot == {"observed": 8 * (40 + 3 * (n_edge - 2 + 2 * n_pods)), "invalid": 8 * 3 * 2, "out_of_group": 8 * 4,
                   "pod_out_of_range": 8 * 3 * 4, "pair_overflow": 0}


@pytest.mark.parametrize("H", [1, 2])
def test_horizons_that_wrap_with_an_empty_step_and_a_step_without_groups(H):
    rng = np.random.default_rng(20 + H)
    G = 4
    groups = [G, G, G, 0, G, G]
    wins = [sc.edge_window(rng, n, G) if n else np.zeros(0, R.SPAN) for n in (30, 25, 0, 35, 10, 45)]
    dev, ref = _pair(3, H, G)
    tot = _run(dev, ref, wins, groups)
    assert tot["observed"] > 100 and tot["out_of_group"] >= 10
    # steps 2 (empty) and 3 (no groups) fill a horizon of up to two windows with nothing
    assert not ref.results(3, G)["rec_pods"].any() and not ref.results(3, G)["rec_n"].any()
    assert ref.results(4, G)["rec_k_top"].any()


@pytest.mark.parametrize("lds", [True, False])
def test_one_hot_pair_and_one_wide_group(lds):
    rng = np.random.default_rng(5)
    v = rng.lognormal(np.log(600.0), 1.0, 4096).astype(np.float32)
    hot = sc.pod_spans(v, np.zeros(4096, np.int64), np.full(4096, 9))
    wide = sc.pod_spans(v, np.ones(4096, np.int64), np.repeat(np.arange(100, 164), 64)[rng.permutation(4096)])
    dev, ref = _pair(3, 2, 2, span_cap=4096, lds=lds)
    try:
        r = _equal_step(dev, ref, hot, 2, f"one pair lds={lds}")
        row = r["win_top"][0][0]
        assert int(r["win_pods"][0]) == 1 and int(row["n"]) == 4096 and int(row["b"]) == int((v > np.float32(800)).sum())
        assert row["max_ttft"] == v.max() and int(row["pod_id"]) == 9
        r = _equal_step(dev, ref, wide, 2, f"64 pods lds={lds}")
        assert int(r["win_pods"][1]) == 64 and int(r["rec_pods"][0]) == 1 and int(r["rec_n"].sum()) == 8192
        assert (r["win_top"][1]["n"] == 64).all()
    finally:
        dev.close()


def test_eight_pairs_that_collide_on_the_tables_last_slot_wrap_around():
    cap = 8
    slots = pr.window_slots(cap)
    assert slots == 16
    pods = sc.colliding_pods(0, slots, slots - 1, cap)
    rng = np.random.default_rng(8)
    recs = sc.pod_spans(rng.choice([100.0, 900.0], 64), np.zeros(64, np.int64), np.repeat(pods, 8)[rng.permutation(64)])
    for lds in (True, False):
        dev, ref = _pair(8, 2, 1, span_cap=64, pair_cap=cap, lds=lds)
        try:
            r = _equal_step(dev, ref, recs, 1, f"colliding lds={lds}")
            assert int(r["win_pods"][0]) == cap and int(r["stats"][4]) == 0
            r = _equal_step(dev, ref, recs[::-1], 1, f"colliding again lds={lds}")
            assert int(r["rec_pods"][0]) == cap and int(r["rec_n"][0]) == 128
        finally:
            dev.close()


@pytest.mark.parametrize("lds", [True, False])
def test_exactly_pair_cap_pairs_equal_the_oracle_and_five_more_keep_the_invariants(lds):
    cap = 8
    exact = sc.pod_spans([900.0, 10.0, 950.0] * cap, [0] * (3 * cap), np.repeat(np.arange(1, cap + 1), 3))
    more = sc.pod_spans([900.0, 10.0, 950.0] * (cap + 5), [0] * (3 * (cap + 5)), np.repeat(np.arange(1, cap + 6), 3))
    dev, ref = _pair(3, 2, 1, span_cap=64, pair_cap=cap, lds=lds)
    try:
        r = _equal_step(dev, ref, exact, 1, "exactly pair_cap")
        assert int(r["win_pods"][0]) == cap and int(r["stats"][4]) == 0
        i = dev.step_records(more, 1)
        assert i == ref.step_records(more, 1) and ref.overflowed(i)
        r = dev.results(i, 1)
        tot, pairs, _ = sc.brute_pairs(more, 1)
        held = dev.resident()
        sc.overflow_invariants(r, pairs, tot, held[i % 2], cap, f"past pair_cap lds={lds}")
        # the horizon's totals do not depend on the pair table; the earlier list is untouched
        assert int(r["rec_n"][0]) == 3 * cap + 3 * (cap + 5) and int(r["rec_b"][0]) == 2 * cap + 2 * (cap + 5)
        sc.same_resident(held[:1], ref.resident()[:1], "the list of the step before")
        # the step after is exact again: nothing of the overflow lingers in the window's table
        i = dev.step_records(exact, 1)
        assert i == ref.step_records(exact, 1)
        a, b = dev.results(i, 1), ref.results(i, 1)
        for key in ("win_n", "win_b", "win_pods", "win_pods_b", "win_k_top", "rec_n", "rec_b", "stats"):
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)
        sc.same_rows(a["win_top"], b["win_top"], "the step after the overflow")
    finally:
        dev.close()


@pytest.mark.parametrize("lds", [True, False])
def test_a_spread_over_both_sides_of_the_lds_group_limit(lds):
    rng = np.random.default_rng(29)
    C = 130
    dev, ref = _pair(3, 2, C, span_cap=2048, pair_cap=1024, lds=lds)
    L = 64  # podrank_host.h kLdsGroups: totals, pod counts and K slots of the services below it sit in LDS
    assert dev.lds_slots == 256 and L < C
    grp = rng.integers(0, C, 2048)
    grp[:60] = np.repeat([L - 1, L, L + 1], 20)  # the services on, at and past the limit hold more than K pods
    pods = 1 + rng.integers(0, 6, 2048)
    wide = sc.pod_spans(rng.lognormal(np.log(700.0), 1.0, 2048), grp, pods)
    try:
        r = _equal_step(dev, ref, wide, C, f"130 services lds={lds}")
        assert int(r["win_n"].sum()) == 2048 and (r["win_k_top"][L - 1:L + 2] == 3).all()
        # n_groups on the limit, one below and one above it
        for G in (L, L - 1, L + 1):
            r = _equal_step(dev, ref, wide[:700], G, f"n_groups = {G} lds={lds}")
            assert int(r["stats"][2]) == int((wide["group_id"][:700] >= G).sum()) > 0
    finally:
        dev.close()


def test_records_split_over_three_ranges():
    rng = np.random.default_rng(33)
    G = 3
    recs = np.ascontiguousarray(sc.edge_window(rng, 60, G))
    n = len(recs)
    a = recs.ctypes.data
    dev, ref = _pair(3, 2, G, span_cap=256)
    try:
        r = _equal_step(dev, ref, recs, G, "three ranges",
                        ranges=[(a, 40 * 64), (a + 40 * 64, 0), (a + 40 * 64, 50 * 64), (a + 90 * 64, (n - 90) * 64)])
        assert int(r["stats"][0]) > 90
        with pytest.raises(ValueError):
            dev.step([(a, 63)], G)
        with pytest.raises(ValueError):
            dev.step_records(recs[:1], G + 1)
        with pytest.raises(ValueError):
            dev.step([(a, 200 * 64), (a, 57 * 64)], G)
        _equal_step(dev, ref, recs[:17], G, "the step after the refused ones")
        assert min(dev.step_ms(1)) >= 0.0 and dev.observe_ms(1) >= 0.0 and dev.query(1)
    finally:
        dev.close()


def test_argument_checks():
    from llm_slo_ebpf_toolkit_amd.ops.podrank import PodRankTracker

    for kw in (dict(k=0), dict(k=9), dict(windows=0), dict(windows=17), dict(group_cap=0), dict(group_cap=65537),
               dict(span_cap=0), dict(span_cap=1 << 22), dict(n_buffers=0), dict(n_buffers=65), dict(pair_cap=0),
               dict(pair_cap=(1 << 20) + 1), dict(slo_ms=-1.0), dict(slo_ms=float("nan"))):
        with pytest.raises(ValueError):
            PodRankTracker(**kw)
    from llm_slo_ebpf_toolkit_amd.ops import load_agent

    mod = load_agent()
    for g, pod, slots in ((0, 0, 2), (3, 77, 8192), (65535, (1 << 20) - 1, 1 << 25)):
        assert int(mod.podrank_slot_of(g, pod, slots)) == pr.slot_of(g, pod, slots)


def test_n_groups_changing_between_steps():
    rng = np.random.default_rng(44)
    C = 6
    groups = [6, 2, 0, 5, 1, 6, 3]
    wins = [sc.edge_window(rng, 50, C) for _ in groups]
    tot = _run(*_pair(3, 3, C, pair_cap=512), wins, groups)
    assert tot["out_of_group"] > 300 and tot["observed"] > 300


def test_randomised_thirty_steps_over_five_groups_and_forty_pods():
    rng = np.random.default_rng(7)
    C = 5
    K, H = 3, 4
    groups = rng.integers(0, C + 1, 30).tolist()
    wins = []
    for g in groups:
        w = sc.window(rng, int(rng.integers(0, 301)), g, C, edges=bool(rng.integers(0, 2)), skipped=bool(rng.integers(0, 2)))
        wins.append(sc.with_pods(w, rng.integers(0, 40, len(w))))
    tot = _run(*_pair(K, H, C, span_cap=512), wins, groups)
    assert tot["observed"] > 1000


def test_through_the_pipeline_and_the_rings_equals_the_host_engine():
    rng = np.random.default_rng(41)
    groups = [3, 3, 2, 3, 1, 3]
    wins = [sc.edge_window(rng, int(n), 3) if n else np.zeros(0, R.SPAN) for n in (30, 50, 20, 0, 25, 60)]
    gpu, gp = sc.run_pipeline("gpu", wins, groups, 3)
    cpu, cp = sc.run_pipeline("cpu", wins, groups, 3)
    off, _ = sc.run_pipeline("gpu", wins, groups, 0)
    for w, (a, b, c, x, y) in enumerate(zip(gpu, cpu, off, gp, cp)):
        assert set(a) == set(b) == set(c) | set(pr.RESULT_KEYS)
        for key in pr.RESULT_KEYS:
            if key in ("pod_win_top", "pod_rec_top"):
                sc.same_rows(a[key], b[key], f"window {w} {key}")
            else:
                np.testing.assert_array_equal(a[key], b[key], err_msg=f"window {w} {key}")
        sc.same_results(x, y, f"window {w}")
        for key in c:  # every other key: the same run with the feature off
            np.testing.assert_array_equal(a[key], c[key], err_msg=f"window {w} {key}")
    assert sum(int(r["pod_win_n"].sum()) for r in gpu) > 150
