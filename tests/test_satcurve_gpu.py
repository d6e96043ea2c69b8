"""The saturation curve tracker on the device (ops/csrc/satcurve.hip) against the host implementation
(pipeline/satcurve.py): the same windows through both, step by step -- the result block as bytes, the
results over group_cap and over n_groups, and everything resident (the three cell arrays, carry, both
generations and their epochs, age, q_hi, q_first) must be equal. The named cases of
tests/satcurve_scenarios.py (interval geometry, every placement and validity case with and without a
TTFT, the levels at 15/16, 16/17 and 8191, advances by 0, 1, several and B or more bins, the fold at
q_first, late records, epoch boundaries, dropped generations, the knee rule's ties and equalities, every
state, age, both refused steps; the hot cases with the LDS table on and off), the bound helpers against
the oracle's, records split over ranges, every refusal, and the whole way through WindowPipeline and the
rings against the host engine."""

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.pipeline import satcurve as sat
from tests import satcurve_scenarios as sc

pytestmark = pytest.mark.gpu


def _pair(cfg, lds=True, **kw):
    from llm_slo_ebpf_toolkit_amd.ops.satcurve import SaturationTracker

    kw = dict(cfg, **kw)
    return SaturationTracker(lds=lds, **kw), sat.SaturationOracle(**kw)


def _equal_step(dev, ref, recs, cut, G, what, ranges=None):
    i = dev.step_records(recs, cut, G) if ranges is None else dev.step(ranges, cut, G)
    assert i == ref.step_records(recs, cut, G)
    a, b = dev.block(i), ref.block(i)
    assert a.dtype == b.dtype == np.uint32 and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: blocks differ"
    a, b = dev.results(i, dev.group_cap), ref.results(i, ref.group_cap)
    sc.same_results(a, b, what)
    sc.same_results(dev.results(i, G), ref.results(i, G), what)
    sc.same_resident(dev.resident(), ref.resident(), what)
    return a


def _run_case(c, lds=True):
    dev, ref = _pair(c.cfg, lds=lds)
    seen, resid = [], []
    try:
        for w, (recs, cut, G) in enumerate(c.steps):
            what = f"{c.name} lds={lds} step {w}"
            if w in c.refused:
                before = dev.resident()
                with pytest.raises(ValueError, match=c.refused[w]):
                    dev.step_records(recs, cut, G)
                with pytest.raises(ValueError, match=c.refused[w]):
                    ref.step_records(recs, cut, G)
                sc.same_resident(dev.resident(), before, what)
                seen.append(None), resid.append(before)
                continue
            seen.append(_equal_step(dev, ref, recs, cut, G, what))
            resid.append(dev.resident())
    finally:
        dev.close()
    if c.check is not None:
        c.check(seen, resid)


@pytest.mark.parametrize("name", [n for n in sc.CASE_NAMES if not n.startswith("hot")])
def test_every_named_case_equals_the_oracle_after_every_step(name):
    _run_case(sc.case(name))


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("name", [n for n in sc.CASE_NAMES if n.startswith("hot")])
def test_hot_cells_with_and_without_the_lds_table(name, lds):
    _run_case(sc.case(name), lds=lds)


def test_the_bound_helpers_equal_the_oracle_s():
    from llm_slo_ebpf_toolkit_amd.ops import load_agent

    mod = load_agent()
    assert int(mod.SATCURVE_LDS_SLOTS) == 256 and int(mod.SATCURVE_ROW_BYTES) == sat.ROW_BYTES == sat.SAT_ROW.itemsize
    assert int(mod.SATCURVE_LEVELS) == sat.K and int(mod.SATCURVE_CURVE_RECORDS_MAX) == sat.MAX_CURVE_RECORDS
    for g in (1, 3, 4, 64, 1000, 65536):
        assert dict(mod.satcurve_layout(g)) == sat.layout(g)
    for shape in ((1024, 16384, 64), (64, 256, 3), (8192, 1, 4096)):
        assert int(mod.satcurve_device_bytes(*shape)) == sat.device_bytes(*shape)
    # the level rule over every u, at both edges of every u, and at the bound's extreme
    for bin_us in (1000, 500_000, 60_000_000):
        for u in list(range(0, 40)) + [255, 256, 4095, 4096, 8190, 8191, 8192, 20000]:
            for busy in {max(0, -(-u * bin_us // 8) - 1), -(-u * bin_us // 8), (u + 1) * bin_us // 8}:
                got = tuple(int(x) for x in mod.satcurve_level(busy, bin_us))
                want = int(sat.u_of(busy, bin_us))
                assert got == (want, int(sat.level_of_u(want))), (bin_us, u, busy, got)
    assert tuple(mod.satcurve_level(1 << 53, 1000)) == (8191, 159) and tuple(mod.satcurve_level(-5, 1000)) == (0, 0)
    for level in range(sat.K + 1):
        assert int(mod.satcurve_lower(level)) == int(sat.lower(level))
    assert all(int(sat.level_of_u(int(sat.lower(l)))) == l for l in range(sat.K))
    # the knee in 64 bits against Python's integers, random curves and the bound's extremes
    rng = np.random.default_rng(4)
    curves = []
    for _ in range(200):
        c = np.zeros((sat.K, 2), np.uint64)
        at = rng.choice(sat.K, int(rng.integers(1, 12)), replace=False)
        c[at, 0] = rng.integers(1, 1000, len(at))
        c[at, 1] = (c[at, 0] * rng.random(len(at)) * rng.choice([0.0, 0.05, 0.3], len(at))).astype(np.uint64)
        curves.append((c, int(rng.choice([1, 10_000, 100_000, 999_999])), int(rng.integers(1, 500))))
    top = np.zeros((sat.K, 2), np.uint64)
    top[159] = (1 << 40, 1 << 40)
    low = np.zeros((sat.K, 2), np.uint64)
    low[0], low[159] = ((1 << 40) - 1, 0), (1, 1)
    curves += [(top, 1, (1 << 31) - 1), (top, 999_999, 1), (low, 999_999, 1), (low, 1, 2), (np.zeros((sat.K, 2), np.uint64), 10_000, 1)]
    for c, budget, min_requests in curves:
        assert tuple(mod.satcurve_knee(c, budget, min_requests)) == sat.knee_of(c.tolist(), budget, min_requests)
    for x in ((True, 10, 4, True, 5, 5), (True, 10, 4, True, 4, 5), (True, 3, 4, True, 9, 5), (False, 10, 4, True, 9, 5),
              (True, 10, 4, False, 9, sat.NONE), (True, 4, 4, False, 0, sat.NONE)):
        assert int(mod.satcurve_state(*x)) == sat.state_of(*x), x
    for x in ((3, 0), (3, 7), (3, 2 ** 32 - 1), (3, 2 ** 32 - 2), (2, 9), (0, 9), (1, 9)):
        assert int(mod.satcurve_age(*x)) == sat.age_of(*x), x
    q = sc.QF
    for x in ((-1, q, -1, 64), (q, q, q, 64), (q, q + 1, q, 64), (q + 5, q + 30, q, 64), (q + 5, q + 69, q, 64),
              (q + 5, q + 500, q, 64), (q + 70, q + 80, q + 40, 64), (q + 5, q + 2000, q - 7, 1024)):
        assert tuple(int(v) for v in mod.satcurve_fold(*x)) == sat.fold_of(*x), x
    # the two populations against the oracle's deques
    o = sat.SaturationOracle(**sc._cfg(epoch_bins=128))
    steps = [(q, 5), (q + 10, 7), (q + 70, 11), (q + 130, 13), (q + 300, 17), (q + 390, 19)]
    for i, (qh, n) in enumerate(steps):
        assert int(mod.satcurve_ring_after(64, steps[:i], qh, n)) == o.ring_after(qh, n)
        assert int(mod.satcurve_curve_after(128, steps[:i], qh, n)) == o.curve_after(qh, n)
        o.step_records(sc.traffic(0, qh - 1, qh - 1, n, 0.1), sc.cut_of(qh), 1)
    assert o.curve_after(q + 390, 0) == 13 + 17 + 19 and o.ring_after(q + 390, 0) == 19


def test_records_split_over_three_ranges_and_every_refused_step():
    c = sc._random("ranges", 3, 33, 6, 120, span_cap=256)
    cut = max(cut for _, cut, _ in c.steps)  # the steps' records in one: late, too old and clipped ones among them
    recs = np.ascontiguousarray(np.concatenate([r for r, _, _ in c.steps])[:150])
    n, G = len(recs), 3
    assert n == 150
    a = recs.ctypes.data
    q = (cut // 1000) // sc.BIN
    dev, ref = _pair(sc._cfg(span_cap=256), ring_records_max=2 * n - 1)
    try:
        r = _equal_step(dev, ref, recs, cut, G, "three ranges",
                        ranges=[(a, 40 * 64), (a + 40 * 64, 0), (a + 40 * 64, 50 * 64), (a + 90 * 64, (n - 90) * 64)])
        assert int(r["stats"][0]) > 50
        before = dev.resident()
        for bad in (lambda: dev.step([(a, 63)], cut, G), lambda: dev.step_records(recs[:1], cut, G + 1),
                    lambda: dev.step_records(recs[:1], cut, -1), lambda: dev.step_records(recs[:1], 0, G),
                    lambda: dev.step_records(recs[:1], -5, G), lambda: dev.step([(a, 200 * 64), (a, 57 * 64)], cut, G),
                    lambda: dev.step([(0, 64)], cut, G),
                    lambda: dev.step_records(recs, sc.cut_of(q + 63), G)):  # 2 n spans in the ring: one too many
            with pytest.raises(ValueError):
                bad()
        sc.same_resident(dev.resident(), before, "a refused step changes nothing")
        _equal_step(dev, ref, recs[:17], sc.cut_of(q + 3), G, "the step after the refused ones")
        _equal_step(dev, ref, recs, sc.cut_of(q + 64 + 3), G, "the first steps expired: room for all n again")
        assert min(dev.step_ms(2)) >= 0.0 and dev.observe_ms(2) >= 0.0 and dev.query(2)
        with pytest.raises(IndexError):
            dev.results(-1, G)
        with pytest.raises(IndexError):
            ref.results(-1, G)
    finally:
        dev.close()


def test_argument_checks():
    from llm_slo_ebpf_toolkit_amd.ops.satcurve import SaturationTracker
    from tests.test_satcurve import BAD_CONFIGS

    for kw in BAD_CONFIGS:
        with pytest.raises(ValueError):
            SaturationTracker(**kw)


def test_through_the_pipeline_and_the_rings_equals_the_host_engine():
    from tests.test_satcurve import _windows

    rng = np.random.default_rng(41)
    groups = [3, 3, 2, 3, 1, 3]
    wins, cuts = _windows(rng)
    cuts[4] = 0  # a cut without a time: skipped and counted
    gpu, go, gskip = sc.run_pipeline("gpu", wins, cuts, groups, 64)
    cpu, co, cskip = sc.run_pipeline("cpu", wins, cuts, groups, 64)
    off, _, _ = sc.run_pipeline("gpu", wins, cuts, groups, 0)
    assert gskip == cskip == 1
    for w, (a, b, c, x, y) in enumerate(zip(gpu, cpu, off, go, co)):
        assert set(a) == set(b) == set(c) | set(sat.RESULT_KEYS)
        sc.same_rows(a["sat_rows"], b["sat_rows"], f"window {w}")
        np.testing.assert_array_equal(a["sat_curve"], b["sat_curve"], err_msg=f"window {w}")
        np.testing.assert_array_equal(a["sat_stats"], b["sat_stats"], err_msg=f"window {w}")
        sc.same_results(x, y, f"window {w}")
        for key in c:  # every other key: the same run with the feature off
            assert np.asarray(a[key]).tobytes() == np.asarray(c[key]).tobytes(), f"window {w} {key}"
    sc.same_results(go[4], sat.empty_result(groups[4]), "the window without a cut time")
    assert int(gpu[5]["sat_rows"]["n_total"].sum()) > 40 and int(gpu[5]["sat_stats"][0]) > 20
