"""The load SLI tracker on the device (ops/csrc/loadsli.hip) against the host implementation
(pipeline/loadsli.py): the same windows through both, step by step -- the result block as bytes, the
results over group_cap and over n_groups, and everything resident (both cell arrays, carry, age, the
previous state, q_hi, q_first) must be equal. The named cases of tests/loadsli_scenarios.py (interval
geometry, every placement and validity case, advances by 0, 1, several and B or more bins, late records,
a start evicted before its end, peak ties inside a lane and across lanes, every state, the three compares
at and one below equality, age, the refused step at the population bound; the hot cases with the LDS
table on and off), the bound helpers against the oracle's, records split over ranges, every refusal, and
the whole way through WindowPipeline and the rings against the host engine."""

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.pipeline import loadsli as ld
from tests import loadsli_scenarios as sc

pytestmark = pytest.mark.gpu


def _pair(cfg, lds=True, **kw):
    from llm_slo_ebpf_toolkit_amd.ops.loadsli import LoadSliTracker

    kw = dict(cfg, **kw)
    return LoadSliTracker(lds=lds, **kw), ld.LoadSliOracle(**kw)


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
                with pytest.raises(ValueError, match="ring_records_max"):
                    dev.step_records(recs, cut, G)
                with pytest.raises(ValueError, match="ring_records_max"):
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
    assert int(mod.LOADSLI_LDS_SLOTS) == 256 and int(mod.LOADSLI_ROW_BYTES) == ld.ROW_BYTES == ld.LOAD_ROW.itemsize
    for x, want in sc.DUR_PATTERNS:
        assert int(mod.loadsli_dur_us(float(np.float32(x)))) == want == int(ld.dur_us(np.float32(x)))
    for bad in (float("nan"), -1.0, float("inf"), float(np.nextafter(np.float32(sc.DAY_MS), np.float32(np.inf)))):
        assert int(mod.loadsli_dur_us(bad)) == -1
    for g in (1, 3, 4, 64, 1000, 65536):
        assert dict(mod.loadsli_layout(g)) == ld.layout(g)
    for shape in ((1024, 16384, 64), (64, 256, 3), (8192, 1, 65536)):
        assert int(mod.loadsli_device_bytes(*shape)) == ld.device_bytes(*shape)
    for shape in ((1024, 500_000), (64, 1000), (8192, 60_000_000), (128, 1000)):
        assert int(mod.loadsli_ring_records_max(*shape)) == ld.default_ring_records_max(*shape)
    # the compares at their bounds' extremes, C++ in 64 bits against Python's integers
    top, n31 = 1 << 53, (1 << 31) - 1
    rng = np.random.default_rng(2)
    cases = [(6000, 8000, 8, 8, 8, 4, 1000, 1500, 4, 500), (6000, 8000, 8, 8, 8, 4, 1000, 1501, 100, 500),
             (0, 0, 4, 12, 8, 4, 1000, 1500, 4, 500), (0, 0, 6, 8, 8, 4, 1000, 1500, 4, 500),
             (top, top, n31, n31, 8191, 8191, 60_000_000, 64000, n31, 10 ** 9), (top, 0, n31, 0, 1, 8191, 60_000_000, 64000, 1, 1),
             (min(top, n31 * 1000), top, n31, n31, 8191, 1, 1000, 64000, 20, 1000)]
    for _ in range(200):
        nb, nr, bu = int(rng.integers(1, 8192)), int(rng.integers(1, 8192)), int(rng.integers(1000, 60_000_001))
        cases.append((int(rng.integers(0, min(top, n31 * nr * bu) + 1)), int(rng.integers(0, min(top, n31 * nb * bu) + 1)),
                      int(rng.integers(0, n31 + 1)), int(rng.integers(0, n31 + 1)), nb, nr, bu, int(rng.integers(1001, 64001)),
                      int(rng.integers(1, 100)), int(rng.integers(1, 5000))))
    for c in cases:
        assert tuple(mod.loadsli_classify(*c)) == ld.classify(*c), c
    for x in ((1, 0, 0), (1, 1, 1), (3, 1, 9), (0, 0, 7), (4, 4, 7), (2, 2, 2 ** 32 - 1), (2, 2, 2 ** 32 - 2)):
        assert int(mod.loadsli_age(*x)) == ld.age_of(*x), x
    q_hi = sc.QH
    for ts, dur in ((q_hi * 1000 + 5, 300), ((q_hi + 2) * 1000, 10), ((q_hi - 1) * 1000 + 300, 5000), ((q_hi - 70) * 1000, 2000),
                    ((q_hi - 70) * 1000 + 500, 10000), ((q_hi - 5) * 1000 + 500, 500)):
        bits, qs, qe, idle_s, idle_e = mod.loadsli_place(ts, dur, 1000, q_hi, 64)
        o = ld.LoadSliOracle(**sc._cfg(64, group_cap=1))
        r = o.results(o.step_records(sc.reqs([0], [ts], [dur / 1000.0]), sc.cut_of(q_hi), 1), 1)
        st = ld.stats_dict(r["stats"])
        assert (bool(bits & 1), bool(bits & 2), bool(bits & 4)) == (st["future"] == 1, st["too_old"] == 1, st["clipped"] == 1)
        res = o.resident()
        assert int(res["idle_us"].sum()) == (idle_s if bits & 8 else 0) + (idle_e if bits & 16 else 0)
        if bits & 16:
            assert int(res["counts"][0, qe & 63]) >> 32 == 1
        if bits & 8:
            assert int(res["counts"][0, qs & 63]) & 0xFFFFFFFF == 1


def test_records_split_over_three_ranges_and_every_refused_step():
    c = sc._random("ranges", 64, 3, 33, 6, 120, span_cap=256)
    cut = max(cut for _, cut, _ in c.steps)  # the steps' records in one: late, too old and clipped ones among them
    recs = np.ascontiguousarray(np.concatenate([r for r, _, _ in c.steps])[:150])
    n, G = len(recs), 3
    assert n == 150
    a = recs.ctypes.data
    q = (cut // 1000) // sc.BIN
    dev, ref = _pair(sc._cfg(64, span_cap=256), ring_records_max=2 * n - 1)
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
    from llm_slo_ebpf_toolkit_amd.ops.loadsli import LoadSliTracker
    from tests.test_loadsli import BAD_CONFIGS

    for kw in BAD_CONFIGS:
        with pytest.raises(ValueError):
            LoadSliTracker(**kw)


def test_through_the_pipeline_and_the_rings_equals_the_host_engine():
    from tests.test_loadsli import _windows

    rng = np.random.default_rng(41)
    groups = [3, 3, 2, 3, 1, 3]
    wins, cuts = _windows(rng)
    cuts[4] = 0  # a cut without a time: skipped and counted
    gpu, go, gskip = sc.run_pipeline("gpu", wins, cuts, groups, 64)
    cpu, co, cskip = sc.run_pipeline("cpu", wins, cuts, groups, 64)
    off, _, _ = sc.run_pipeline("gpu", wins, cuts, groups, 0)
    assert gskip == cskip == 1
    for w, (a, b, c, x, y) in enumerate(zip(gpu, cpu, off, go, co)):
        assert set(a) == set(b) == set(c) | set(ld.RESULT_KEYS)
        sc.same_rows(a["load_rows"], b["load_rows"], f"window {w}")
        np.testing.assert_array_equal(a["load_stats"], b["load_stats"], err_msg=f"window {w}")
        sc.same_results(x, y, f"window {w}")
        for key in c:  # every other key: the same run with the feature off
            assert np.asarray(a[key]).tobytes() == np.asarray(c[key]).tobytes(), f"window {w} {key}"
    sc.same_results(go[4], ld.empty_result(groups[4]), "the window without a cut time")
    assert int(gpu[5]["load_rows"]["arr_ring"].sum()) > 40 and int(gpu[5]["load_stats"][0]) > 20
