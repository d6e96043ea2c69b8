"""Overlapped windows (ops/csrc/engine.hip, "window overlap"): a window runs as a front stage
(head, reset, definitions, decode, span side, signal scatter, probe work list) and a back stage
(probe .. packet) on two streams, so window k + 1's front runs beside window k's back. Every
array both stages touch is per buffer or per physical generation slot (docs/ARCHITECTURE.md).

Checked here, window by window, over a stress sequence that alternates full and nearly empty
windows (each stage in turn the long one) and holds a window without spans and one without
events: the overlapped engine against the numpy oracle (the existing rules: exact counts, rtol
1e-9 on posteriors) and against an engine built with MISLO_WINDOW_OVERLAP=0 (byte-identical
packets and result blocks: every sum is an integer atomic and the posterior is deterministic).
Windows are staged ahead of the read-back (RingWindowSource keeps n_buffers - 1 in flight), so
front(k + 1) is queued while back(k) may still run."""

import dataclasses
import os

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.models.bayes import NaiveBayes
from llm_slo_ebpf_toolkit_amd.pipeline import oracle
from llm_slo_ebpf_toolkit_amd.pipeline.replay import ReplayConfig, ReplayGenerator

pytestmark = pytest.mark.gpu

HALO_MS = 4000.0   # windows are 1 s apart: rows of windows k-1, k-2 and k-3 stay visible
INT64_MAX = (1 << 63) - 1
# F full, E nearly empty, S no spans, Z no events (a window without local records ends the halo chain)
SEQUENCE = "FEFEFFEFSFEZFEFEFF"
RES_KEYS = ("post", "gconf", "feat", "pred", "evbits", "sli")


def _rings(tag, user_rec=64):
    from llm_slo_ebpf_toolkit_amd.runtime import load

    rt = load()
    return (rt.Ringbuf.create_shm(f"/mislo-ov-{os.getpid()}-{tag}", 1 << 22), rt.HostRing(1 << 14, user_rec),
            rt.HostRing(1 << 12, 64))


def _feed(img, rb, user, spans):
    from llm_slo_ebpf_toolkit_amd.pipeline.window import Cut

    assert rb.append_framed(img.framed)
    assert user.push(img.user) == len(img.user)
    assert spans.push(img.spans) == len(img.spans)
    return Cut(kernel=rb.producer_pos, user=user.head, spans=spans.head, bases=img.bases)


def _pod_meta(gen):
    sn = (gen.pod_svc.astype(np.uint32) << np.uint32(16)) | gen.pod_node.astype(np.uint32)
    return gen.pod_ids.astype(np.uint32), sn


def _stress_windows(seq=SEQUENCE, seed=53):
    cfg = ReplayConfig(scenario="full", n_nodes=2, pods_per_node=8, n_services=8, events_per_window=8192,
                       spans_per_window=512, seed=seed)
    gen = ReplayGenerator(cfg)
    wins = []
    for kind in seq:
        w = gen.next_window()
        if kind == "E":
            w = dataclasses.replace(w, events=np.ascontiguousarray(w.events[:96]), spans=np.ascontiguousarray(w.spans[:8]))
        elif kind == "S":
            w = dataclasses.replace(w, spans=np.ascontiguousarray(w.spans[:0]))
        elif kind == "Z":
            w = dataclasses.replace(w, events=np.ascontiguousarray(w.events[:0]))
        wins.append(w)
    return wins, gen


@pytest.fixture(scope="module")
def stress():
    """The stress sequence, its ring images and the oracle's per-window reference, computed once."""
    from llm_slo_ebpf_toolkit_amd.parallel.exchange import ExchangeModel
    from llm_slo_ebpf_toolkit_amd.pipeline.window import build_replay_images

    wins, gen = _stress_windows()
    imgs = build_replay_images(wins)
    pods, sn = _pod_meta(gen)
    pod_sn = dict(zip(pods.tolist(), sn.tolist()))
    table, tmap = oracle.CtxTable(), oracle.TraceMap()
    xm = ExchangeModel(0, 1, HALO_MS, 0, 0, halo_windows=3)
    refs = []
    for w, img in zip(wins, imgs):
        oracle.apply_ring_defs(img.framed, table, tmap, pod_sn)
        d = oracle.decode_window(img.framed, img.user, table, tmap, img.bases, pod_sn=pod_sn)
        n_halo = len(xm.halo().ts)
        ref = xm.join(d, oracle.spans_native(img.spans, tmap), w.n_groups)
        refs.append({"hist": oracle.histograms(d), "sums": oracle.value_sums_milli(d), "join": ref, "n_halo": n_halo,
                     "n_loc": len(d.ts), "events": R.framed_event_count(img.framed) + len(img.user)})
    return wins, imgs, (pods, sn), refs


def _run(tag, imgs, pods, overlap, use_graphs, n_buffers, cuts=None, **kw):
    """The sequence through one engine, windows staged ahead of the read-back: per window the raw
    packet and result block (copies). ``cuts``: a list receiving import_state()'s per-age
    cut-offs after every staged window (the query drains the engine, so no two windows of such
    a run overlap in time; what it may not do is change what a later window computes)."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import RingWindowSource, WindowPipeline

    old = os.environ.get("MISLO_WINDOW_OVERLAP")
    os.environ["MISLO_WINDOW_OVERLAP"] = "1" if overlap else "0"
    try:
        pipe = WindowPipeline(16384, 512, 8, model="bayes", learn=False, user_cap=4096, halo_ms=HALO_MS,
                              use_graphs=use_graphs, n_buffers=n_buffers, max_ahead=n_buffers, **kw)
    finally:
        if old is None:
            del os.environ["MISLO_WINDOW_OVERLAP"]
        else:
            os.environ["MISLO_WINDOW_OVERLAP"] = old
    rb, user, spans = _rings(tag)
    src = RingWindowSource(pipe, rb, user, spans)
    pipe.eng.set_pods(*pods)
    out = []

    def collect(k, n_groups):
        pipe.eng.wait(k)
        res = pipe.eng.results(k, n_groups)
        out.append((np.array(pipe.eng.packet(k), copy=True), {key: np.array(res[key], copy=True) for key in res}))

    ks = []
    for j, img in enumerate(imgs):
        ks.append(src.stage(_feed(img, rb, user, spans), img.n_groups, img.labels)["k"])
        if cuts is not None:
            cuts.append([int(x) for x in pipe.eng.import_state()[6:10]])
        if j >= 1:  # window j - 1's host blocks are not rewritten before window j - 1 + n_buffers
            collect(ks[j - 1], imgs[j - 1].n_groups)
    collect(ks[-1], imgs[-1].n_groups)
    src.drain()
    state = [int(x) for x in pipe.eng.import_state()]
    graphs = pipe.eng.graphs
    pipe.close()
    return out, state, graphs


@pytest.mark.parametrize("n_buffers", [2, 3])
@pytest.mark.parametrize("use_graphs", [True, False])
def test_overlapped_windows_match_oracle_and_serial_engine(stress, use_graphs, n_buffers):
    from llm_slo_ebpf_toolkit_amd.pipeline.window import unpack_packet

    wins, imgs, pods, refs = stress
    assert len(imgs) >= 16
    tag = f"{int(use_graphs)}{n_buffers}"
    cuts = []
    ser, ser_state, _ = _run("s" + tag, imgs, pods, False, use_graphs, n_buffers, cuts=cuts)
    ovl, ovl_state, graphs = _run("o" + tag, imgs, pods, True, use_graphs, n_buffers)
    # precondition: rows three windows old were visible somewhere (the slot rotation is observable)
    assert any(c[0] == -(1 << 63) and c[3] != INT64_MAX for c in cuts), cuts
    assert any(r["n_halo"] > 0 for r in refs)
    assert ser_state[3] == 4 and ovl_state[3] == 4  # four logical generations in both
    assert ovl_state[6:14] == ser_state[6:14]       # the same cut-offs and rows per age at the end
    if use_graphs:
        assert graphs >= 2 * n_buffers  # a front and a back graph per buffer
    model = NaiveBayes.ref()
    for j, (w, img, ref) in enumerate(zip(wins, imgs, refs)):
        pk_raw, res = ovl[j]
        pk = unpack_packet(pk_raw)
        msg = f"window {j} ({SEQUENCE[j]})"
        np.testing.assert_array_equal(pk["hist"].astype(np.int64), ref["hist"], err_msg=msg)
        np.testing.assert_array_equal(pk["misc"][2:18].astype(np.int64), ref["sums"], err_msg=msg)
        assert pk["ring_state"]["first_busy"] == -1 and pk["ring_state"]["events"] == ref["events"], msg
        dbg = pk["dbg"][:5].astype(np.int64).tolist()
        jr = ref["join"]
        assert (dbg[0], dbg[3], dbg[4]) == (jr.debug["candidates"], jr.debug["fanout_dropped"],
                                            jr.debug["spans_enriched"]), msg
        np.testing.assert_array_equal(res["feat"], jr.feat, err_msg=msg)
        feat = res["feat"].astype(np.float64)
        np.testing.assert_allclose(res["post"][:, :10], model.posteriors(feat), rtol=1e-9, atol=1e-12, err_msg=msg)
        np.testing.assert_array_equal(res["pred"], np.argmax(model.logits(feat), axis=1), err_msg=msg)
        conf = np.zeros((16, 16), dtype=np.int64)
        np.add.at(conf, (img.labels, res["pred"]), 1)
        np.testing.assert_array_equal(pk["confusion"].astype(np.int64), conf, err_msg=msg)
        exp = np.zeros((w.n_groups, 2), dtype=np.int64)
        np.add.at(exp[:, 0], w.spans["group_id"], 1)
        np.add.at(exp[:, 1], w.spans["group_id"], (w.spans["ttft_ms"] > 800.0).astype(np.int64))
        np.testing.assert_array_equal(res["sli"].astype(np.int64), exp, err_msg=msg)
        # the serial engine: nothing may differ
        assert pk_raw.tobytes() == ser[j][0].tobytes(), msg
        assert sorted(res) == sorted(ser[j][1])
        for key in res:
            assert res[key].tobytes() == ser[j][1][key].tobytes(), (msg, key)


@pytest.mark.parametrize("n_buffers", [2, 3])
def test_import_state_between_windows_disturbs_no_later_window(stress, n_buffers):
    """import_state() after every staged window of the overlapped engine (graphs on: from a
    buffer's third use its stages are replayed, not re-run): the diagnostic reads the latest
    window's buffer and changes nothing, so every window's packet and result arrays are the bytes
    of the same engine run without the queries, and the per-age cut-offs it returns window by
    window are the serial engine's."""
    _, imgs, pods, _ = stress
    tag = f"q{n_buffers}"
    ser_cuts, ovl_cuts = [], []
    _run("s" + tag, imgs, pods, False, True, n_buffers, cuts=ser_cuts)
    plain, plain_state, _ = _run("p" + tag, imgs, pods, True, True, n_buffers)
    asked, asked_state, graphs = _run("a" + tag, imgs, pods, True, True, n_buffers, cuts=ovl_cuts)
    assert graphs >= 2 * n_buffers  # the stages were replayed from captured graphs
    assert len(ovl_cuts) == len(imgs) and ovl_cuts == ser_cuts
    # precondition: rows three windows old were visible somewhere
    assert any(c[0] == -(1 << 63) and c[3] != INT64_MAX for c in ovl_cuts), ovl_cuts
    assert asked_state == plain_state
    assert len(asked) == len(plain) == len(imgs)
    for j in range(len(imgs)):
        msg = f"window {j} ({SEQUENCE[j]})"
        assert asked[j][0].tobytes() == plain[j][0].tobytes(), msg
        assert sorted(asked[j][1]) == sorted(plain[j][1])
        for key in asked[j][1]:
            assert asked[j][1][key].tobytes() == plain[j][1][key].tobytes(), (msg, key)


def test_overlap_with_the_span_side_on_its_own_stream(stress, monkeypatch):
    """MISLO_SPAN_STREAM=1 with overlapped windows (not the default: the front stage's graph then
    forks the span side onto the side stream and joins it before the stage ends) computes the same
    windows as the serial engine."""
    _, imgs, pods, _ = stress
    ser, _, _ = _run("bs", imgs, pods, False, True, 3)
    monkeypatch.setenv("MISLO_SPAN_STREAM", "1")
    ovl, _, _ = _run("bo", imgs, pods, True, True, 3)
    for j in range(len(imgs)):
        assert ovl[j][0].tobytes() == ser[j][0].tobytes(), j
        for key in ovl[j][1]:
            assert ovl[j][1][key].tobytes() == ser[j][1][key].tobytes(), (j, key)


def test_communicator_switches_the_overlap_off_and_keeps_the_buffer_sets(stress):
    """An engine built with the overlap on that then gets a communicator (one rank here) runs the
    serial chain on the compute stream over the per-buffer sets and the spare generation slot it
    allocated: the same windows as an engine built with MISLO_WINDOW_OVERLAP=0, and import_state()
    (which drains the compute stream as well as the comm stream) ends on the same cut-offs."""
    from llm_slo_ebpf_toolkit_amd.ops import load_agent

    _, imgs, pods, _ = stress
    ser, ser_state, _ = _run("cs", imgs, pods, False, True, 3, comm=(load_agent().unique_id(), 0, 1))
    hyb, hyb_state, _ = _run("ch", imgs, pods, True, True, 3, comm=(load_agent().unique_id(), 0, 1))
    assert hyb_state[6:14] == ser_state[6:14]
    for j in range(len(imgs)):
        assert hyb[j][0].tobytes() == ser[j][0].tobytes(), j
        for key in hyb[j][1]:
            assert hyb[j][1][key].tobytes() == ser[j][1][key].tobytes(), (j, key)


def _learn_run(tag, imgs, pods, overlap):
    from llm_slo_ebpf_toolkit_amd.pipeline.window import RingWindowSource, WindowPipeline

    old = os.environ.get("MISLO_WINDOW_OVERLAP")
    os.environ["MISLO_WINDOW_OVERLAP"] = "1" if overlap else "0"
    try:
        pipe = WindowPipeline(16384, 512, 8, model="bayes_learned", learn=True, user_cap=4096, halo_ms=HALO_MS)
    finally:
        if old is None:
            del os.environ["MISLO_WINDOW_OVERLAP"]
        else:
            os.environ["MISLO_WINDOW_OVERLAP"] = old
    rb, user, spans = _rings(tag)
    src = RingWindowSource(pipe, rb, user, spans)
    pipe.eng.set_pods(*pods)
    packets = []
    for img in imgs[:7]:  # labelled windows: statistics, the prequential refit n_buffers behind
        src.stage(_feed(img, rb, user, spans), img.n_groups, img.labels, with_labels=True, learn=True)
    pipe.eng.refit_now()  # from the statistics folded so far, stream-ordered behind the queued back stages
    pipe.eng.set_device_refit(False)  # the model stays frozen while scoring
    ks = []
    for img in imgs[7:12]:  # scoring with the refitted model
        ks.append(src.stage(_feed(img, rb, user, spans), img.n_groups, img.labels, with_labels=True, learn=False)["k"])
        if len(ks) >= 2:
            pipe.eng.wait(ks[-2])
            packets.append(np.array(pipe.eng.packet(ks[-2]), copy=True))
    pipe.eng.wait(ks[-1])
    packets.append(np.array(pipe.eng.packet(ks[-1]), copy=True))
    src.drain()
    model = np.array(pipe.eng.model_bytes(), copy=True)
    stats = np.array(pipe.eng.stats_acc(), copy=True)
    folded = pipe.windows_folded
    pipe.close()
    return model, stats, packets, folded


def test_learning_then_refit_gives_the_serial_engines_model(stress):
    """learn=True windows, refit_now, then scoring: the refit and the per-window prequential refit
    stay on the back stage's stream, so the model bytes, the accumulated statistics and the scored
    packets equal the serial engine's."""
    _, imgs, pods, _ = stress
    m_s, st_s, pk_s, f_s = _learn_run("ls", imgs, pods, False)
    m_o, st_o, pk_o, f_o = _learn_run("lo", imgs, pods, True)
    assert f_s == f_o and f_s > 0
    assert st_o.tobytes() == st_s.tobytes() and np.abs(st_s).sum() > 0
    assert m_o.tobytes() == m_s.tobytes()
    assert len(pk_o) == len(pk_s) == 5
    for j, (a, b) in enumerate(zip(pk_o, pk_s)):
        assert a.tobytes() == b.tobytes(), j


def test_model_bytes_after_refit_now_with_a_communicator(stress):
    """With a communicator the comm stream is a stream of its own, and refit_now runs on the
    compute stream: model_bytes() right behind it must drain that stream too and return the
    refitted model -- the one a second read after a full drain returns, not the initial one."""
    from llm_slo_ebpf_toolkit_amd.ops import load_agent
    from llm_slo_ebpf_toolkit_amd.pipeline.window import RingWindowSource, WindowPipeline

    _, imgs, pods, _ = stress
    pipe = WindowPipeline(16384, 512, 8, model="bayes_learned", learn=True, user_cap=4096, halo_ms=HALO_MS,
                          comm=(load_agent().unique_id(), 0, 1))
    rb, user, spans = _rings("cm")
    src = RingWindowSource(pipe, rb, user, spans)
    pipe.eng.set_pods(*pods)
    first = np.array(pipe.eng.model_bytes(), copy=True)
    for img in imgs[:7]:
        src.stage(_feed(img, rb, user, spans), img.n_groups, img.labels, with_labels=True, learn=True)
    pipe.eng.set_device_refit(False)
    pipe.eng.refit_now()
    now = np.array(pipe.eng.model_bytes(), copy=True)
    src.drain()
    later = np.array(pipe.eng.model_bytes(), copy=True)
    pipe.close()
    assert now.tobytes() == later.tobytes()
    assert now.tobytes() != first.tobytes()


def _pods_run(tag, imgs, pods, overlap, change_at):
    from llm_slo_ebpf_toolkit_amd.pipeline.window import RingWindowSource, WindowPipeline

    old = os.environ.get("MISLO_WINDOW_OVERLAP")
    os.environ["MISLO_WINDOW_OVERLAP"] = "1" if overlap else "0"
    try:
        pipe = WindowPipeline(16384, 512, 8, model="bayes", learn=False, user_cap=4096)
    finally:
        if old is None:
            del os.environ["MISLO_WINDOW_OVERLAP"]
        else:
            os.environ["MISLO_WINDOW_OVERLAP"] = old
    rb, user, spans = _rings(tag, 24)
    src = RingWindowSource(pipe, rb, user, spans)
    ids, sn = pods
    pipe.eng.set_pods(ids, sn)
    out, ks = [], []

    def collect(k, n_groups):  # the packet and the incident features, as bytes
        pipe.eng.wait(k)
        out.append(np.array(pipe.eng.packet(k), copy=True).tobytes() + pipe.eng.results(k, n_groups)["feat"].tobytes())

    for j, img in enumerate(imgs):
        if j == change_at:  # every pod moves to the next service: queued behind the windows in flight
            svc = ((sn >> np.uint32(16)) + np.uint32(1)) % np.uint32(8)
            pipe.eng.set_pods(ids, (svc << np.uint32(16)) | (sn & np.uint32(0xFFFF)))
        ks.append(src.stage(_feed(img, rb, user, spans), img.n_groups, img.labels)["k"])
        if j >= 1:
            collect(ks[j - 1], imgs[j - 1].n_groups)
    collect(ks[-1], imgs[-1].n_groups)
    src.drain()
    pipe.close()
    return out


def test_set_pods_takes_effect_at_the_next_submitted_window():
    """The pod table is read by the front stage (definitions, decode of USER24 records): an upload
    between two submits lands between their front stages, exactly as in the serial engine -- the
    windows before it keep the old services, the windows from it on get the new ones."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import build_replay_images

    wins, gen = _stress_windows("FFFFFF", seed=59)
    imgs = build_replay_images(wins, user_rec=24)
    pods = _pod_meta(gen)
    ser = _pods_run("ps", imgs, pods, False, 3)
    ovl = _pods_run("po", imgs, pods, True, 3)
    same = _pods_run("pn", imgs, pods, True, None)
    for j in range(len(imgs)):
        assert ovl[j] == ser[j], j
    for j in range(3):
        assert ovl[j] == same[j], j
    assert ovl[3] != same[3]  # the change is visible in the window it precedes
