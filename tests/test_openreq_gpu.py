"""The open-request table on the device (ops/csrc/openreq.hip) against the host implementation
(pipeline/openreq.py): the same request streams through both, step by step -- the per-group
deadline counts and corrections, the statistics and the live rows must be equal. Small and crowded
tables, an overfull one (conservation only: which insert loses is unordered), the global-atomic
path above the LDS group limit, a randomised stress, and the whole way through WindowPipeline and
the rings against the host engine."""

import os

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.collector import records as R
from tests import openreq_scenarios as sc

pytestmark = pytest.mark.gpu


def _pair(cap, group_cap=8, span_cap=16384, **kw):
    from llm_slo_ebpf_toolkit_amd.ops.openreq import OpenRequestTable
    from llm_slo_ebpf_toolkit_amd.pipeline.openreq import OpenRequestOracle

    kw = dict(cap=cap, span_cap=span_cap, group_cap=group_cap, slo_ms=sc.SLO_MS, reorder_ms=2000.0, **kw)
    return OpenRequestTable(**kw), OpenRequestOracle(**kw)


def _equal_every_step(st, dev, ref, probes=False):
    """Both trackers over the stream; returns the summed statistics."""
    from llm_slo_ebpf_toolkit_amd.pipeline.openreq import MAX_PROBES, unordered_traces

    total = np.zeros(16, np.int64)
    excluded = 0
    prev = 0
    for w, (spans, cut) in enumerate(zip(st.windows, st.cuts)):
        excluded += unordered_traces(spans)
        a = dev.results(dev.step_records(spans, cut, prev, st.n_groups), st.n_groups)
        b = ref.results(ref.step_records(spans, cut, prev, st.n_groups), st.n_groups)
        prev = cut
        for key in ("dl", "dup", "stats"):
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"window {w} {key}")
        for x, y, name in zip(dev.entries(), ref.entries(), ("trace_h", "t", "grp", "state")):
            np.testing.assert_array_equal(x, y, err_msg=f"window {w} entries {name}")
        if probes:
            assert ref.probe_lengths().max(initial=0) <= MAX_PROBES
        total += a["stats"].astype(np.int64)
    assert excluded == 0  # no trace with two counted records in one window (their order is not defined)
    return total


def test_small_table_equals_the_oracle_after_every_step():
    st = sc.stream(seed=17, n_groups=3, per_window=5, n_windows=13, send_windows=8, fault_window=3, fault_group=1)
    assert st.n_requests == 40 and st.n_breaching > 3
    dev, ref = _pair(64)
    try:
        tot = _equal_every_step(st, dev, ref)
    finally:
        dev.close()
    assert tot[2] == 0 and ref.entries()[0].size == 0  # nothing dropped; every request reported


def test_crowded_table_with_long_probe_chains():
    """48 requests open at once in 64 slots (plus the rows removed within a step, which hold their
    slot until its end): probe chains run long, nothing is dropped."""
    from llm_slo_ebpf_toolkit_amd.pipeline.openreq import OpenRequestOracle

    st = sc.stream(seed=3, n_groups=3, per_window=48, n_windows=8, send_windows=1, fault_window=0, fault_group=0,
                   healthy_ms=1500.0, late_ms=4200.0)
    dev, ref = _pair(64)
    try:
        tot = _equal_every_step(st, dev, ref, probes=True)  # the host rows' probe lengths stay <= 64
    finally:
        dev.close()
    peak = max(int(r["stats"][5:8].sum()) for r in sc.run(OpenRequestOracle(cap=64, slo_ms=sc.SLO_MS), st))
    assert peak == 48 and tot[2] == 0 and tot[10] == 0


def test_overfull_table_drops_starts_and_still_conserves():
    """200 requests open at once, 64 slots. The service pushes its records itself (none carries
    SPAN_LATE): the engine counts a breach that is flagged late in ``late`` alone, not among the
    requests of any window, so with untracked requests only an unflagged stream has a request sum
    to conserve."""
    from llm_slo_ebpf_toolkit_amd.pipeline.openreq import correct_results

    st = sc.stream(seed=4, n_groups=3, per_window=200, n_windows=8, send_windows=1, fault_window=0, fault_group=2,
                   healthy_ms=1300.0, late_ms=3500.0, flag_late=False)
    dev, _ = _pair(64)
    try:
        cor, dropped = [], 0
        prev = 0
        for spans, cut in zip(st.windows, st.cuts):
            r = dev.results(dev.step_records(spans, cut, prev, st.n_groups), st.n_groups)
            prev = cut
            sli, late = sc.engine_counts(spans, st.n_groups)
            cor.append(correct_results({"sli": sli, "late": late}, r))
            dropped += int(r["stats"][2])
            assert int(r["stats"][5:8].sum()) <= 64
    finally:
        dev.close()
    assert dropped > 0
    # a dropped start is a request counted when it reports, as without the tracker: still once
    assert sum(int(c["sli"][:, 0].sum()) for c in cor) == st.n_requests
    assert sum(int(c["sli"][:, 1].sum()) + int(c["late"][:, 0].sum()) for c in cor) == st.n_breaching


def test_global_atomic_path_above_the_lds_group_limit():
    from llm_slo_ebpf_toolkit_amd.ops import load_agent

    G = int(load_agent().OPENREQ_LDS_GROUPS) + 1
    st = sc.stream(seed=8, n_groups=G, per_window=400, n_windows=10, send_windows=5, fault_window=1,
                   fault_group=G - 1, healthy_ms=950.0)  # every request breaches: all groups count
    assert st.n_requests == 2000
    dev, ref = _pair(1 << 12, group_cap=G)
    try:
        tot = _equal_every_step(st, dev, ref)
    finally:
        dev.close()
    assert tot[2] == 0 and ref.entries()[0].size == 0


def test_the_lds_path_at_its_limit_equals_the_oracle():
    from llm_slo_ebpf_toolkit_amd.ops import load_agent

    G = int(load_agent().OPENREQ_LDS_GROUPS)
    st = sc.stream(seed=9, n_groups=G, per_window=300, n_windows=8, send_windows=3, fault_window=1,
                   fault_group=G - 1, healthy_ms=950.0)
    dev, ref = _pair(1 << 12, group_cap=G)
    try:
        _equal_every_step(st, dev, ref)
    finally:
        dev.close()


def test_randomised_stress():
    from llm_slo_ebpf_toolkit_amd.pipeline.openreq import EVENT_STATS, STATS

    rng = np.random.default_rng(21)
    st = sc.stream(seed=21, n_groups=7, per_window=715, n_windows=12, send_windows=7, fault_window=2, fault_group=3)
    assert st.n_requests >= 5000
    # what the generator's service never does: duplicate starts; first tokens of requests that never
    # said "started", whose start records come a window later (dropped by the markers); requests
    # that start again after they reported (counted at the deadline, never reported: they expire);
    # counted requests that report a TTFT within the SLO after all; records without a trace or
    # outside the groups
    orphans = np.zeros(0, R.SPAN)
    for w in range(1, 10):
        spans = st.windows[w].copy()
        ft = (spans["flags"] & R.SPAN_FIRST_TOKEN) != 0
        slow = np.nonzero(ft & (spans["ttft_ms"] > sc.SLO_MS))[0][:2]
        spans["ttft_ms"][slow] = 700.0
        extra = []
        starts = spans[(spans["flags"] & R.SPAN_START) != 0]
        if len(starts):
            extra.append(starts[rng.integers(0, len(starts), 20)])
        old = st.windows[w - 1]
        old = old[((old["flags"] & R.SPAN_FIRST_TOKEN) != 0) & (old["ttft_ms"] < sc.SLO_MS)]
        for recs in (orphans, old[rng.integers(0, len(old), 10)] if len(old) else old):
            again = recs.copy()
            again["flags"], again["ttft_ms"] = R.SPAN_START | R.SPAN_NO_SLI, np.nan
            extra.append(again)
        orphans = spans[ft][:10].copy()
        orphans["trace_h"] = rng.integers(1 << 62, 1 << 63, len(orphans)).astype(np.uint64)
        orphans["flags"] = R.SPAN_FIRST_TOKEN
        extra.append(orphans)
        junk = spans[:6].copy()
        junk["trace_h"][:3] = 0
        junk["trace_h"][3:] = rng.integers(1, 1 << 62, 3).astype(np.uint64)
        junk["group_id"][3:] = 99
        extra.append(junk)
        allrec = np.concatenate([spans] + extra)
        st.windows[w] = allrec[rng.permutation(len(allrec))]
    dev, ref = _pair(1 << 14, ttl_ms=4000.0)
    try:
        tot = dict(zip(STATS, _equal_every_step(st, dev, ref).tolist()))
    finally:
        dev.close()
    assert all(tot[k] > 0 for k in EVENT_STATS if k != "dropped_full"), tot
    assert tot["dropped_full"] == 0 and tot["marker_dropped"] == 0


def test_argument_checks_and_result_slots():
    from llm_slo_ebpf_toolkit_amd.ops.openreq import OpenRequestTable

    with pytest.raises(ValueError):
        OpenRequestTable(cap=100)
    with pytest.raises(ValueError):
        OpenRequestTable(cap=64, slo_ms=0.0)
    t = OpenRequestTable(cap=64, span_cap=4, group_cap=2, n_buffers=2)
    try:
        none = np.zeros(0, R.SPAN)
        with pytest.raises(ValueError):
            t.step_records(none, 0, 0, 2)
        with pytest.raises(ValueError):
            t.step_records(none, 10, 20, 2)
        with pytest.raises(ValueError):
            t.step_records(none, 10, 0, 3)
        with pytest.raises(ValueError):
            t.step_records(np.zeros(5, R.SPAN), 10, 0, 2)
        with pytest.raises(ValueError):
            t.step([(1 << 20, 63)], 10, 0, 2)
        for i in range(3):
            assert t.step_records(none, sc.cut_of(i), 0, 2) == i
        assert t.results(2, 2)["dl"].shape == (2, 2) and t.results(1, 2)["dup"].shape == (2, 3)
        with pytest.raises(IndexError):
            t.results(0, 2)
        assert min(t.step_ms(2)) >= 0.0
    finally:
        t.close()


def test_through_the_pipeline_and_the_rings_equals_the_host_engine():
    st = sc.stream(seed=5, n_groups=3, per_window=30, n_windows=14, fault_window=5, fault_group=1)
    gpu, gstats, gc = sc.run_pipeline("gpu", st, f"org{os.getpid()}")
    cpu, cstats, cc = sc.run_pipeline("cpu", st, f"orh{os.getpid()}")
    assert gc == cc == {"skipped": 1}
    for w, (a, b) in enumerate(zip(gpu, cpu)):
        assert set(a) == set(b)
        for key in ("sli", "late", "sli_raw", "late_raw", "deadline", "deadline_dup"):
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"window {w} {key}")
        np.testing.assert_array_equal(gstats[w], cstats[w], err_msg=f"window {w} stats")
    first = min(w for w, r in enumerate(gpu) if r["sli"][:, 1].any() or r["late"][:, 0].any())
    first_raw = min(w for w, r in enumerate(gpu) if r["sli_raw"][:, 1].any() or r["late_raw"][:, 0].any())
    assert first <= st.fault_window + 1 and first_raw >= st.fault_window + 3
    assert sum(int(r["sli"][:, 0].sum()) for r in gpu) == st.n_requests
    assert sum(int(r["sli"][:, 1].sum()) + int(r["late"][:, 0].sum()) for r in gpu) == st.n_breaching
