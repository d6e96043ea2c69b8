"""The decode SLI tracker on the device (ops/csrc/decodesli.hip) against the host implementation
(pipeline/decodesli.py): the same windows through both, step by step -- the whole result block (as bytes),
every field over group_cap and over n_groups, and the resident rolling state must be equal. The named
cases of tests/decodesli_scenarios.py (every bucket edge, ranks on a lane's last and the next lane's first
bucket, n = 1, both sides of both SLOs, the order of the checks, what is skipped, horizons of two and three
windows with a window leaving, empty steps, changing group counts and a service going silent; one hot
cell, three adjacent buckets, more keys than the LDS table holds and a randomised run with the LDS table on
and off), records split over ranges, every refusal, and the whole way through WindowPipeline and the rings
against the host engine."""

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.pipeline import decodesli as ds
from tests import decodesli_scenarios as sc

pytestmark = pytest.mark.gpu


def _pair(cfg, lds=True, **kw):
    from llm_slo_ebpf_toolkit_amd.ops.decodesli import DecodeSliTracker

    kw = dict(cfg, **kw)
    return DecodeSliTracker(lds=lds, **kw), ds.DecodeSliOracle(**kw)


def _equal_step(dev, ref, recs, G, what, ranges=None):
    i = dev.step_records(recs, G) if ranges is None else dev.step(ranges, G)
    assert i == ref.step_records(recs, G)
    assert dev.block(i).tobytes() == ref.block(i).tobytes(), f"{what}: result blocks differ"
    a, b = dev.results(i, dev.group_cap), ref.results(i, ref.group_cap)
    sc.same_results(a, b, what)
    sc.same_results(dev.results(i, G), ref.results(i, G), what)
    sc.same_resident(dev.resident(), ref.resident(), what)
    return a


def _run_case(c, lds=True):
    dev, ref = _pair(c.cfg, lds=lds)
    seen = []
    try:
        assert dev.tpot_slo_us == ref.tpot_slo_us == sc.SLO_US
        for w, (recs, G) in enumerate(c.steps):
            seen.append(_equal_step(dev, ref, recs, G, f"{c.name} lds={lds} step {w}"))
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


def test_the_device_bucket_rule_is_the_oracle_s():
    from llm_slo_ebpf_toolkit_amd.ops import load_agent

    mod = load_agent()
    assert mod.DECODESLI_LDS_SLOTS == 256
    for u in sc.EDGE_US + [100_000, 98_303, 98_304, 102_399, 102_400]:
        assert mod.decodesli_bucket_of(u) == int(ds.bucket_of(u)) == sc.brute_bucket(u), u


def test_records_split_over_three_ranges_and_every_refused_step():
    rng = np.random.default_rng(33)
    G = 3
    recs = np.ascontiguousarray(sc.mixed_window(rng, 120, G))
    n = len(recs)
    assert 150 < n <= 256
    a = recs.ctypes.data
    dev, ref = _pair(sc._cfg(span_cap=256))
    try:
        r = _equal_step(dev, ref, recs, G, "three ranges",
                        ranges=[(a, 40 * 64), (a + 40 * 64, 0), (a + 40 * 64, 50 * 64), (a + 90 * 64, (n - 90) * 64)])
        assert int(r["stats"][0]) > 90
        before = dev.resident()
        for bad in (lambda: dev.step([(a, 63)], G), lambda: dev.step_records(recs[:1], G + 1),
                    lambda: dev.step_records(recs[:1], -1), lambda: dev.step([(a, 200 * 64), (a, 57 * 64)], G),
                    lambda: dev.step([(0, 64)], G)):
            with pytest.raises(ValueError):
                bad()
        for bad in (lambda: ref.step([(a, 63)], G), lambda: ref.step_records(recs[:1], G + 1),
                    lambda: ref.step_records(recs[:1], -1), lambda: ref.step_records(np.concatenate([recs, recs]), G),
                    lambda: ref.step([(0, 64)], G)):
            with pytest.raises(ValueError):
                bad()
        sc.same_resident(dev.resident(), before, "a refused step changes nothing")
        _equal_step(dev, ref, recs[:17], G, "the step after the refused ones")
        _equal_step(dev, ref, recs[:0], G, "an empty step: no observe launch")
        assert min(dev.step_ms(2)) >= 0.0 and dev.observe_ms(1) >= 0.0 and dev.query(2)
        with pytest.raises(IndexError):
            ref.results(-1, G)
        with pytest.raises(IndexError):
            dev.results(-1, G)
    finally:
        dev.close()


def test_argument_checks():
    from llm_slo_ebpf_toolkit_amd.ops.decodesli import DecodeSliTracker

    for kw in (dict(windows=0), dict(windows=4097), dict(group_cap=0), dict(group_cap=65537), dict(span_cap=0),
               dict(n_buffers=0), dict(n_buffers=65), dict(slo_ms=-1.0), dict(slo_ms=float("nan")), dict(slo_ms=float("inf")),
               dict(tpot_slo_ms=0.0), dict(tpot_slo_ms=-1.0), dict(tpot_slo_ms=float("nan")), dict(tpot_slo_ms=float("inf")),
               dict(span_cap=1 << 21, windows=2048), dict(group_cap=65536, windows=4096)):
        with pytest.raises(ValueError):
            DecodeSliTracker(**kw)
        with pytest.raises(ValueError):
            ds.DecodeSliOracle(**kw)


def test_through_the_pipeline_and_the_rings_equals_the_host_engine():
    rng = np.random.default_rng(41)
    groups = [3, 3, 2, 3, 1, 3]
    wins = [sc.mixed_window(rng, 40, 3) if w != 3 else np.zeros(0, sc.R.SPAN) for w in range(6)]
    gpu, gd = sc.run_pipeline("gpu", wins, groups, 2)
    cpu, cd = sc.run_pipeline("cpu", wins, groups, 2)
    off, _ = sc.run_pipeline("gpu", wins, groups, 0)
    for w, (a, b, c, x, y) in enumerate(zip(gpu, cpu, off, gd, cd)):
        assert set(a) == set(b) == set(c) | set(ds.RESULT_KEYS) and not set(c) & set(ds.RESULT_KEYS)
        sc.same_results(x, y, f"window {w}")
        for key in ds.RESULT_KEYS:
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"window {w} {key}")
        for key in c:  # every other key: the same run with the feature off
            np.testing.assert_array_equal(a[key], c[key], err_msg=f"window {w} {key}")
    assert int(gd[3]["cells"].sum()) == 0 and int(gd[3]["cells_roll"].sum()) > 30
    assert sum(int(r["decode_cells"].sum()) for r in gpu) > 200
