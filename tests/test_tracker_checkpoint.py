"""Checkpoint and resume of the side trackers' horizons, the parts that need no device
(docs/TRACKER_CHECKPOINT.md): every numpy oracle's ``state`` / ``restore`` round trip against an oracle that
was never interrupted, the fingerprint's refusals by field name, ``WindowPipeline`` on the CPU engine (state
keys, the gap's empty steps, a gap as long as the horizon).

The shapes are the smallest at which a horizon carries something: horizon 3 (``windows=3``; drift ``recent=1,
gap=1, baseline=2``; error sli one pair over 3 windows; the time rings 64 bins), two result buffers, a span
buffer of 8 records, two groups. Steps: ``w, w, w, empty | state, restore into a new oracle | empty, w, empty,
w``, a second between cuts. ``test_a_fresh_oracle_differs`` keeps the round trip honest: without it an oracle
that forgot everything would pass too. tests/test_tracker_checkpoint_gpu.py holds the same on the device."""

import importlib
import inspect
import json

import numpy as np
import pytest

from tests.test_steplane_gpu import GROUP_CAP, N_BUFFERS, SECOND_NS, SPAN_CAP, TRACKERS, _one_pair, same_results

BEFORE, AFTER = 4, 4   # steps before the checkpoint (the last one empty) and after it (empty, w, empty, w)
EMPTY = (3, 4, 6)      # the steps without a record


def _horizon(name, sc):
    """The tracker's sizes at horizon 3 (the time rings keep their 64 bins)."""
    kw = dict(TRACKERS[name][3](sc))
    if "windows" in kw:
        kw["windows"] = 3
    if name == "drift":
        kw.update(recent=1, gap=1, baseline=2)
    if name == "errsli":
        kw["pairs"] = ((3, 1, sc.F1),)
    return kw


def _window(name, sc):
    """The window every non-empty step feeds: tests/test_steplane_gpu.py's smallest scenario window, but for
    decode sli its 4-record case (the 1-record one carries nothing the horizon keeps) and for the pod
    breakdown ``edge_window(rng, 2, 2)`` cut to one pair (some one-pair windows hold no breach)."""
    if name == "decodesli":
        return next(s for c in sc.cases() for s in c.steps if len(s[0]) == 4)
    if name == "podrank":
        return (_one_pair(sc.edge_window(np.random.default_rng(11), 2, GROUP_CAP)),)
    return TRACKERS[name][4](sc)


def checkpoint_plan(name):
    """(configuration, [(records, extra step arguments)] of the eight steps) of one tracker."""
    sc = importlib.import_module(f"tests.{TRACKERS[name][2]}")
    takes = TRACKERS[name][5]
    small = _window(name, sc)
    recs = np.ascontiguousarray(small[0][:SPAN_CAP])
    assert 1 <= len(recs) <= SPAN_CAP
    cut0 = int(small[1]) if takes else SECOND_NS
    steps = []
    for w in range(BEFORE + AFTER):
        cut = cut0 + w * SECOND_NS
        extra = {"": (), "cut": (cut,), "cuts": (cut, cut - SECOND_NS if w else 0)}[takes]
        steps.append((recs[:0] if w in EMPTY else recs, extra))
    kw = dict(_horizon(name, sc), n_buffers=N_BUFFERS, span_cap=SPAN_CAP, group_cap=GROUP_CAP)
    return kw, steps


def oracle_class(name):
    rules = importlib.import_module(f"llm_slo_ebpf_toolkit_amd.pipeline.{name}")
    return getattr(rules, TRACKERS[name][1])


def oracle_of(name, **kw):
    return oracle_class(name)(**kw)


_REFERENCE = {}


def reference(name):
    """The uninterrupted oracle's results of the four later steps and its state after step 3, computed once
    and left unchanged: (kw, steps, [results], (arrays, meta))."""
    if name not in _REFERENCE:
        kw, steps = checkpoint_plan(name)
        ref = oracle_of(name, **kw)
        saved, later = None, []
        for w, (recs, extra) in enumerate(steps):
            if w == BEFORE:
                arrays, meta = ref.state()
                saved = ({k: v.copy() for k, v in arrays.items()}, json.loads(json.dumps(meta)))  # as a file carries it
            assert ref.step_records(recs, *extra, GROUP_CAP) == w
            if w >= BEFORE:
                later.append(ref.results(w, GROUP_CAP))
        _REFERENCE[name] = (kw, steps, later, saved)
    return _REFERENCE[name]


def _differs(a, b):
    return any(np.ascontiguousarray(a[k]).tobytes() != np.ascontiguousarray(b[k]).tobytes() for k in a)


@pytest.mark.parametrize("name", list(TRACKERS))
def test_a_fresh_oracle_differs(name):
    """What keeps the round trips honest: an oracle that starts fresh at the checkpoint (but at the same step
    index) does not give the continued oracle's results at the first later step."""
    kw, steps, later, _saved = reference(name)
    fresh = oracle_of(name, **kw)
    recs, extra = steps[BEFORE]
    i = fresh.step_records(recs, *extra, GROUP_CAP)
    assert _differs(fresh.results(i, GROUP_CAP), later[0]), f"{name}: the horizon carries nothing over the checkpoint"


@pytest.mark.parametrize("name", list(TRACKERS))
def test_oracle_round_trip_equals_the_uninterrupted_oracle(name):
    kw, steps, later, (arrays, meta) = reference(name)
    assert set(arrays) == {"image"} and arrays["image"].dtype == np.uint8 and meta["step"] == BEFORE
    new = oracle_of(name, **kw)
    assert new.restore(arrays, meta) == BEFORE
    for i in range(BEFORE):
        with pytest.raises(LookupError):  # IndexError; the open-request oracle's KeyError
            new.results(i, GROUP_CAP)  # the steps before the resumed index are not held
    for w in range(BEFORE, BEFORE + AFTER):
        recs, extra = steps[w]
        assert new.step_records(recs, *extra, GROUP_CAP) == w
        same_results(new.results(w, GROUP_CAP), later[w - BEFORE], f"{name} step {w}")
    with pytest.raises(RuntimeError, match="before the first step"):
        new.restore(arrays, meta)


def _other(name, kw):
    """The fields to vary: (field the refusal names, other configuration)."""
    out = []
    if "windows" in kw:
        out.append(("windows", dict(kw, windows=2, **({"pairs": ((2, 1, kw["pairs"][0][2]),)} if name == "errsli" else {}))))
    if "bins" in kw:
        # the saturation curve's epoch holds at least the ring's bins; bins comes first and is what is named
        out.append(("bins", dict(kw, bins=128, **({"epoch_bins": 128} if "epoch_bins" in kw else {}))))
    if name == "drift":
        out.append(("baseline", dict(kw, baseline=3)))
    out.append(("group_cap", dict(kw, group_cap=GROUP_CAP + 1)))
    # every tracker whose constructor takes an slo_ms, whether or not the shapes above set one
    slo = inspect.signature(oracle_class(name).__init__).parameters.get("slo_ms")
    if slo is not None:
        out.append(("slo_ms", dict(kw, slo_ms=float(kw.get("slo_ms", slo.default)) + 1.0)))
    return out


HAVE_SLO_MS = ("openreq", "podrank", "onset", "decodesli", "satcurve", "retrsli")


def test_every_tracker_with_an_slo_ms_has_it_varied():
    """The refusal test below finds the trackers with an ``slo_ms`` by their constructors: these six."""
    kws = {name: reference(name)[0] for name in TRACKERS}
    assert tuple(n for n in TRACKERS if any(f == "slo_ms" for f, _kw in _other(n, kws[n]))) == HAVE_SLO_MS


@pytest.mark.parametrize("name", list(TRACKERS))
def test_oracle_refuses_another_configuration_by_field_name(name):
    kw, steps, later, (arrays, meta) = reference(name)
    varied = _other(name, kw)
    assert len(varied) >= 2
    for field, other_kw in varied:
        new = oracle_of(name, **other_kw)
        with pytest.raises(ValueError, match=rf"image: {field} "):
            new.restore(arrays, meta)
        # refused means untouched: it steps like a new oracle
        recs, extra = steps[0]
        fresh = oracle_of(name, **other_kw)
        assert new.step_records(recs, *extra, GROUP_CAP) == fresh.step_records(recs, *extra, GROUP_CAP) == 0
        same_results(new.results(0, GROUP_CAP), fresh.results(0, GROUP_CAP), f"{name} after a refusal ({field})")
    # another tracker's state
    other = "errsli" if name != "errsli" else "drift"
    with pytest.raises(ValueError, match="image: kind "):
        oracle_of(name, **kw).restore(*reference(other)[3])
    # an image cut short
    with pytest.raises(ValueError):
        oracle_of(name, **kw).restore({"image": arrays["image"][:-1]}, meta) if len(arrays["image"]) else \
            oracle_of(name, **kw).restore({"image": np.zeros(1, np.uint8)}, meta)


# ---- WindowPipeline, CPU engine -------------------------------------------------------------------------
def _pipeline(**kw):
    from llm_slo_ebpf_toolkit_amd.pipeline.window import WindowPipeline

    return WindowPipeline(1024, SPAN_CAP, GROUP_CAP, model="bayes", learn=False, engine="cpu", n_buffers=N_BUFFERS,
                          window_ms=1000.0, **kw)


def _feed(pipe, name, recs):
    """One window's tracker step, as RingWindowSource does it before the submit."""
    ranges = [(recs.ctypes.data, recs.nbytes)] if len(recs) else []
    {"slisketch": pipe.track_sli, "errsli": pipe.track_errors}[name](ranges, GROUP_CAP)


def test_pipeline_state_without_a_tracker_is_todays():
    pipe = _pipeline()
    arrays, meta = pipe.state()
    assert set(arrays) == {"stats_acc", "model", "host_count", "host_elevated_sum", "host_x_sum", "host_xx"}
    assert set(meta) == {"model", "seed", "learn", "windows", "windows_folded_device", "windows_folded_host", "n_domains"}
    assert pipe.restore(arrays, meta) == {"resumed": [], "fresh": {}}
    pipe.close()


def _two_tracker_pipelines():
    sk, er = reference("slisketch"), reference("errsli")
    on = dict(sli_sketch=3, error_sli=3, error_target=er[0]["target"], error_pairs=er[0]["pairs"],
              error_min_requests=er[0]["min_requests"])
    return sk, er, on


def test_pipeline_state_holds_one_array_per_tracker_and_resumes_over_a_gap(tmp_path):
    sk, er, on = _two_tracker_pipelines()
    a = _pipeline(**on)
    for w in range(BEFORE):
        _feed(a, "slisketch", sk[1][w][0])
        _feed(a, "errsli", er[1][w][0])
    now = 1_700_000_000 * SECOND_NS
    arrays, meta = a.state()
    assert {k for k in arrays if k.startswith("tracker/")} == {"tracker/slisketch", "tracker/errsli"}
    assert set(meta["trackers"]) == {"slisketch", "errsli"} and meta["window_ms"] == 1000.0 and meta["saved_unix_ns"] > 0
    for name in ("slisketch", "errsli"):
        t = meta["trackers"][name]
        assert t["step"] == BEFORE and t["bytes"] == len(arrays[f"tracker/{name}"]) and t["fingerprint"] and t["kind"]
    meta["saved_unix_ns"] = now
    path = str(tmp_path / "state.safetensors")
    from llm_slo_ebpf_toolkit_amd.utils import checkpoint

    checkpoint.save(path, arrays, meta)
    arrays, meta = checkpoint.load(path)

    # one window missed: one empty step, which is the uninterrupted oracles' step 4; then their step 5
    b = _pipeline(**on)
    rep = b.restore(arrays, meta, now_ns=now + 1 * SECOND_NS + 999_999_999)
    assert rep == {"resumed": ["slisketch", "errsli"], "fresh": {}}
    assert b.sketch.n == b.errors.n == BEFORE + 1 and not b._sli and not b._err
    _feed(b, "slisketch", sk[1][5][0])
    _feed(b, "errsli", er[1][5][0])
    same_results(b.sketch.results(5, GROUP_CAP), sk[2][1], "sketch after the gap")
    same_results(b.errors.results(5, GROUP_CAP), er[2][1], "error sli after the gap")
    same_results(b.sli_results(0, GROUP_CAP), sk[2][1], "window 0 of the new pipeline is the sketch's step 5")

    # no window missed: no step
    c = _pipeline(**on)
    assert c.restore(arrays, meta, now_ns=now + SECOND_NS - 1)["resumed"] == ["slisketch", "errsli"]
    assert c.sketch.n == c.errors.n == BEFORE

    # as many missed as the horizon holds: nothing would survive
    d = _pipeline(**on)
    rep = d.restore(arrays, meta, now_ns=now + 3 * SECOND_NS)
    assert rep["resumed"] == [] and set(rep["fresh"]) == {"slisketch", "errsli"}
    assert all("3 windows missed, the horizon holds 3" in r for r in rep["fresh"].values())
    assert d.sketch.n == d.errors.n == 0

    # another horizon: that tracker alone starts fresh, by the field's name; one that is off is not mentioned
    e = _pipeline(sli_sketch=2)
    rep = e.restore(arrays, meta, now_ns=now)
    assert rep["resumed"] == [] and "windows 3, this tracker 2" in rep["fresh"]["slisketch"] and set(rep["fresh"]) == {"slisketch"}
    # a tracker the checkpoint does not hold
    f = _pipeline(decode_sli=3, **on)
    rep = f.restore(arrays, meta, now_ns=now)
    assert rep["resumed"] == ["slisketch", "errsli"] and rep["fresh"] == {"decodesli": "no saved image"}
    for p in (a, b, c, d, e, f):
        p.close()
