"""The breach-onset tracker on the device (ops/csrc/onset.hip) against the host implementation
(pipeline/onset.py): the same windows through both, step by step -- every row of group_cap (as bytes), the
statistics and the whole resident ring must be equal. The named cases of tests/onset_scenarios.py (the
rule's edge values at one and two bins a lane, zeros of S on a lane's last and first bin, the alarm
threshold's two sides, clipped, quiet after a peak, ring wrap, jumping and standing cuts, a late record
that moves the onset back, empty steps and changing group counts, one hot cell and 16 hot cells with the
LDS table on and off, a randomised run), records split over ranges, every refusal, and the whole way
through WindowPipeline and the rings against the host engine."""

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.pipeline import onset as on
from tests import onset_scenarios as sc

pytestmark = pytest.mark.gpu


def _pair(cfg, lds=True, **kw):
    from llm_slo_ebpf_toolkit_amd.ops.onset import OnsetTracker

    kw = dict(cfg, **kw)
    return OnsetTracker(lds=lds, **kw), on.OnsetOracle(**kw)


def _equal_step(dev, ref, recs, cut, G, what, ranges=None):
    i = dev.step_records(recs, cut, G) if ranges is None else dev.step(ranges, cut, G)
    assert i == ref.step_records(recs, cut, G)
    a, b = dev.results(i, dev.group_cap), ref.results(i, ref.group_cap)
    sc.same_results(a, b, what)
    sc.same_results(dev.results(i, G), ref.results(i, G), what)
    sc.same_resident(dev.resident(), ref.resident(), what)
    return a


def _run_case(c, lds=True):
    dev, ref = _pair(c.cfg, lds=lds)
    seen = []
    try:
        for w, (recs, cut, G) in enumerate(c.steps):
            seen.append(_equal_step(dev, ref, recs, cut, G, f"{c.name} lds={lds} step {w}"))
    finally:
        dev.close()
    if c.check is not None:
        c.check(seen)


@pytest.mark.parametrize("name", [n for n in sc.CASE_NAMES if not n.startswith("hot")])
def test_every_named_case_equals_the_oracle_after_every_step(name):
    _run_case(sc.case(name))


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("name", [n for n in sc.CASE_NAMES if n.startswith("hot")])
def test_hot_cells_with_and_without_the_lds_table(name, lds):
    _run_case(sc.case(name), lds=lds)


@pytest.mark.parametrize("lds", [True, False])
def test_more_cells_in_a_workgroup_than_the_lds_table_probes_for(lds):
    # 8 services over 64 bins: 512 (service, slot) keys into a table of 256 slots, so records overflow to the ring
    rng = np.random.default_rng(21)
    B, C, n = 64, 8, 3000
    q_hi = sc.Q0 + 900
    ts = (q_hi - rng.integers(0, B, n)) * sc.BIN + rng.integers(0, sc.BIN, n)
    recs = sc.timed(np.where(rng.random(n) < 0.3, sc.BAD, sc.GOOD), rng.integers(0, C, n), ts)
    dev, ref = _pair(sc._cfg(B, group_cap=C, span_cap=4096), lds=lds)
    try:
        assert dev.lds_slots == 256
        r = _equal_step(dev, ref, recs, sc.cut_of(q_hi), C, f"wide lds={lds}")
        assert int(r["rows"]["n_ring"].sum()) == n
        _equal_step(dev, ref, recs[::-1], sc.cut_of(q_hi + 7), C, f"wide again lds={lds}")
    finally:
        dev.close()


def test_records_split_over_three_ranges_and_every_refused_step():
    rng = np.random.default_rng(33)
    G, B = 3, 64
    q = sc.Q0 + 50
    recs = np.ascontiguousarray(sc.edge_window(rng, 60, G, q, B))
    n = len(recs)
    assert n > 100
    a = recs.ctypes.data
    dev, ref = _pair(sc._cfg(B, span_cap=256), ring_records_max=2 * n - 1)
    try:
        r = _equal_step(dev, ref, recs, sc.cut_of(q), G, "three ranges",
                        ranges=[(a, 40 * 64), (a + 40 * 64, 0), (a + 40 * 64, 50 * 64), (a + 90 * 64, (n - 90) * 64)])
        assert int(r["stats"][0]) > 90
        before = dev.resident()
        for bad in (lambda: dev.step([(a, 63)], sc.cut_of(q), G), lambda: dev.step_records(recs[:1], sc.cut_of(q), G + 1),
                    lambda: dev.step_records(recs[:1], sc.cut_of(q), -1), lambda: dev.step_records(recs[:1], 0, G),
                    lambda: dev.step_records(recs[:1], -5, G), lambda: dev.step([(a, 200 * 64), (a, 57 * 64)], sc.cut_of(q), G),
                    lambda: dev.step_records(recs, sc.cut_of(q + B - 1), G)):  # 2 n spans in the ring: one too many
            with pytest.raises(ValueError):
                bad()
        sc.same_resident(dev.resident(), before, "a refused step changes nothing")
        _equal_step(dev, ref, recs[:17], sc.cut_of(q + 3), G, "the step after the refused ones")
        _equal_step(dev, ref, recs, sc.cut_of(q + B + 3), G, "the first steps expired: room for all n again")
        assert min(dev.step_ms(2)) >= 0.0 and dev.observe_ms(2) >= 0.0 and dev.query(2)
        with pytest.raises(IndexError):
            ref.results(-1, G)
    finally:
        dev.close()


def test_argument_checks():
    from llm_slo_ebpf_toolkit_amd.ops.onset import OnsetTracker

    for kw in (dict(bins=32), dict(bins=16384), dict(bins=96), dict(bin_ns=999_999), dict(bin_ns=60_000_000_001),
               dict(ref_ppm=0), dict(ref_ppm=1_000_000), dict(alarm=0), dict(alarm=1_000_001), dict(group_cap=0),
               dict(group_cap=65537), dict(span_cap=0), dict(n_buffers=0), dict(n_buffers=65), dict(slo_ms=-1.0),
               dict(slo_ms=float("nan")), dict(ring_records_max=0), dict(ring_records_max=1 << 31),
               dict(group_cap=32768, bins=8192)):
        with pytest.raises(ValueError):
            OnsetTracker(**kw)


def test_through_the_pipeline_and_the_rings_equals_the_host_engine():
    rng = np.random.default_rng(41)
    B = 64
    groups = [3, 3, 2, 3, 1, 3]
    qs = [sc.Q0 + sc.PER_WINDOW * (w + 1) for w in range(6)]
    wins = [sc.edge_window(rng, 30, 3, q, B) if w != 3 else np.zeros(0, sc.R.SPAN) for w, q in enumerate(qs)]
    cuts = [sc.cut_of(q) for q in qs]
    cuts[4] = 0  # a cut without a time: skipped and counted
    gpu, go, gskip = sc.run_pipeline("gpu", wins, cuts, groups, B, onset_bin_ns=sc.BIN)
    cpu, co, cskip = sc.run_pipeline("cpu", wins, cuts, groups, B, onset_bin_ns=sc.BIN)
    off, _, _ = sc.run_pipeline("gpu", wins, cuts, groups, 0)
    assert gskip == cskip == 1
    for w, (a, b, c, x, y) in enumerate(zip(gpu, cpu, off, go, co)):
        assert set(a) == set(b) == set(c) | set(on.RESULT_KEYS)
        sc.same_rows(a["onset_rows"], b["onset_rows"], f"window {w}")
        sc.same_results(x, y, f"window {w}")
        for key in c:  # every other key: the same run with the feature off
            np.testing.assert_array_equal(a[key], c[key], err_msg=f"window {w} {key}")
    sc.same_results(go[4], on.empty_result(groups[4]), "the window without a cut time")
    assert sum(int(r["onset_rows"]["n_ring"].sum()) for r in gpu) > 150 and any(int(r["onset_rows"]["state"].max()) == 2 for r in gpu)
