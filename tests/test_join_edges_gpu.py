"""The join kernels (ops/csrc/join.hip) on the hand-built cases of pipeline/join_cases.py against
``oracle.join_bruteforce``: every comparison is exact (keys, integers, and floats both sides compute
by the same operations). Through the kernel harness with every intermediate compared, with
``base_attrs``, through the shipped window engine, and under the probe's diagnostic knobs."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.collector import records
from llm_slo_ebpf_toolkit_amd.pipeline import join_cases, oracle
from tests import join_edges_check as chk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = join_cases.cases()


@pytest.fixture(scope="module")
def harness():
    return chk.make_harness()


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_match_bruteforce(harness, name):
    """top3, cnt, attrs, conf, kernel_ms, group sums and counts (stripe 0 after the fold), features
    and the six debug counters of every case at every one of its parameter sets."""
    assert chk.run_case(harness, name) == len(CASES[name].params)


def test_window_beyond_the_key_packing_is_refused(harness):
    """The top-3 key holds |dt| in 35 bits: 34 s still fits (``boundaries_wide`` runs there), 34.36 s does not."""
    with pytest.raises(ValueError):
        harness.set_join_params(34360.0, 0.7, 3, 1)
    harness.set_join_params(34000.0, 0.7, 3, 1)
    harness.set_join_params()


@pytest.mark.parametrize("group_mode", [1, 0])
def test_base_attrs_are_merged_not_replaced(harness, group_mode):
    """``Engine.join(spans, n_groups, base_attrs)``: the kept candidates are max-merged into the rows
    given ("take if absent or greater", REF's rule replayed over the reference top-3), and group
    mode 0 sums those merged rows."""
    torch = harness.torch
    c = CASES["ranking"]
    S, G = len(c.spans), c.n_groups
    pi = next(i for i, p in enumerate(c.params) if p["group_mode"] == group_mode and p["threshold"] == 0.7)
    p = c.params[pi]
    ref, d = chk.reference("ranking", pi), chk.decoded("ranking")
    rng = np.random.default_rng(7)
    base = rng.uniform(0.0, 300.0, (harness.span_cap, 16)).astype(np.float32)
    base[rng.random(base.shape) < 0.5] = np.nan
    exp = base[:S].copy()
    for s in range(S):
        for key in ref.top3[s][: p["fanout"]]:
            if key == np.uint64(0xFFFFFFFFFFFFFFFF):
                continue
            g = int(key & np.uint64((1 << oracle.SIG_BITS) - 1))
            sl, v = int(d.slot[g]), d.val[g]
            if np.isnan(exp[s, sl]) or v > exp[s, sl]:
                exp[s, sl] = v
    assert (exp != base[:S])[~np.isnan(exp)].any() and (exp == base[:S]).any()
    gsum, gcnt = ref.gsum, ref.gcnt
    if group_mode == 0:
        gsum, gcnt = np.zeros_like(ref.gsum), np.zeros_like(ref.gcnt)
        for s in range(S):
            grp, have = int(c.spans["group_id"][s]), ~np.isnan(exp[s])
            gsum[grp][have] += oracle.milli_units(exp[s][have])
            gcnt[grp][have] += 1
    harness.set_join_params(**p)
    harness.stage(c.events, c.spans, G)
    harness.upload()
    e = harness.eng
    e.reset_window()
    e.decode_wire(harness.ev_dev, 64)
    e.join(harness.sp_dev, G, torch.from_numpy(base).to(harness.device))
    torch.cuda.synchronize(harness.device)
    dbg = e.dbg.cpu().numpy()
    from llm_slo_ebpf_toolkit_amd.ops.engine import decode_debug

    debug = decode_debug(dbg, e.misc.cpu().numpy(), S, len(c.events))
    chk.compare(f"ranking base_attrs {p}", chk.harness_state(harness, S, G), e.feat[:G].cpu().numpy(), debug, ref,
                attrs=exp, gsum=gsum, gcnt=gcnt)
    harness.set_join_params()


SHIPPED = [("boundaries", dict(window_ms=2000.0, threshold=0.7)), ("boundaries", dict(window_ms=100.0, threshold=0.7)),
           ("boundaries", dict(window_ms=300.0, threshold=0.7)), ("precedence", dict(threshold=0.7, fanout=3, group_mode=1)),
           ("precedence", dict(threshold=0.85, fanout=3, group_mode=1)), ("ranking", {}), ("long_lists", {}),
           ("sliced_lists", {}), ("many_groups_65", dict(threshold=0.7, group_mode=1)),
           ("many_groups_65", dict(group_mode=0)), ("many_groups_100", dict(threshold=0.7, group_mode=1)),
           ("many_groups_100", dict(group_mode=0))]


@pytest.fixture(scope="module")
def shipped():
    from llm_slo_ebpf_toolkit_amd.ops.engine import GpuEngine

    eng = GpuEngine(chk.CAPS["sig_cap"], chk.CAPS["span_cap"], chk.CAPS["group_cap"])
    yield eng
    eng.close()


@pytest.mark.parametrize("name,want", SHIPPED, ids=[f"{n}-{i}" for i, (n, _) in enumerate(SHIPPED)])
def test_shipped_engine_matches_bruteforce(shipped, name, want):
    """ops.engine.GpuEngine, the WindowEngine path (signal scatter with the work list in its launch,
    generation metadata, connections folded to 32 bits): features, histograms and the six debug
    counters, twice on one engine so that its buffers are reused. (The 64-bit hash collisions of
    ``mixed_runs`` do not survive the fold and run through the harness only.)"""
    c = CASES[name]
    pi = next(i for i, p in enumerate(c.params) if all(p[k] == v for k, v in want.items()))
    p = c.params[pi]
    ref = chk.reference(name, pi, True)
    hist = oracle.histograms(chk.decoded(name, True))
    shipped.pipe.eng.set_join_params(p["window_ms"], p["threshold"], p["fanout"], p["group_mode"])
    for rep in range(2):
        out = shipped.process(c.events, c.spans, c.n_groups)
        np.testing.assert_array_equal(out.feat, ref.feat, err_msg=f"{name} {p} run {rep}")
        np.testing.assert_array_equal(out.hist, hist)
        for k in chk.DEBUG_KEYS:
            assert out.debug[k] == ref.debug[k], (name, p, rep, k, out.debug[k], ref.debug[k])


@pytest.mark.parametrize("pi", [0, 1], ids=["all-candidates", "top2-attrs"])
def test_halo_rows_at_the_cut_off_and_ties_across_windows(pi):
    """Two windows through a WindowEngine with a 2 s halo (``join_cases.halo_pair``): the second
    window's spans join first-window rows down to the cut-off exactly and no row 1 ns before it, and
    rows of both windows at one |dt| rank this window's first. Reference: ``ExchangeModel.join``;
    features, candidates and enriched spans as in test_halo_and_remote_rows_join_like_the_oracle."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import Cut, RingWindowSource, WindowPipeline
    from llm_slo_ebpf_toolkit_amd.runtime import load as load_rt

    rt = load_rt()
    wins = join_cases.halo_pair()
    p = wins[0].params[pi]
    pipe = WindowPipeline(1024, 64, 8, model="bayes", learn=False, user_cap=1024, n_buffers=2, max_ahead=2,
                          halo_ms=join_cases.HALO_MS, import_cap=1024, **p)
    user, spans = rt.HostRing(4096, 64), rt.HostRing(256, 64)
    src = RingWindowSource(pipe, None, user, spans)
    refs = chk.halo_reference(pi)
    assert refs[0][2] == 0 and refs[1][2] > 0
    for w, (ref, _rows, _n_halo) in zip(wins, refs):
        assert user.push(np.ascontiguousarray(w.events)) == len(w.events)
        assert spans.push(np.ascontiguousarray(w.spans)) == len(w.spans)
        k = src.stage(Cut(kernel=0, user=user.head, spans=spans.head), w.n_groups, None, with_labels=False, learn=False)["k"]
        dbg = pipe.packet(k)["dbg"][:5].astype(np.int64).tolist()
        res = pipe.results(k, w.n_groups)
        src.reap()
        assert (dbg[0], dbg[4]) == (ref.debug["candidates"], ref.debug["spans_enriched"]), (w.name, dbg, ref.debug)
        np.testing.assert_array_equal(res["feat"], ref.feat, err_msg=w.name)
    src.drain()
    pipe.eng.close()


KNOBS = [{"MISLO_PROBE_LDS_GROUPS": "0"},                         # k_probe<256, false>: sums straight to global memory
         {"MISLO_PROBE_ITEM": "16", "MISLO_PROBE_GRID": "3"},     # 7000 signals want 438 slices: the cap of 64 applies
         {"MISLO_PROBE_ITEM": "1000", "MISLO_PROBE_GRID": "1"}]   # one workgroup drains the whole queue


@pytest.mark.parametrize("knobs", KNOBS, ids=["global-groups", "item16-grid3", "item1000-grid1"])
def test_probe_knobs_change_nothing(knobs):
    """The knobs are read once per process: a fresh child per setting runs long_lists, sliced_lists and
    precedence through the harness with the same exact comparison and prints its verdict."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MISLO_PROBE_")}
    env.update(knobs)
    r = subprocess.run([sys.executable, "-m", "tests.join_edges_check", "long_lists", "sliced_lists", "precedence"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    verdict = json.loads(lines[-1])
    assert verdict["ok"] and r.returncode == 0, verdict
    assert verdict["knobs"] == knobs
    assert verdict["runs"] == sum(len(CASES[n].params) for n in ("long_lists", "sliced_lists", "precedence"))
