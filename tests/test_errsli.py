"""The error SLI on the host (pipeline/errsli.py, collector/otlp.py outcome_class): the classification, the
span status through both parsers, the mapper switched off and on, the mask-only claim for the other seven
oracles, the named scenarios against a brute force and their hand-computed expectations, every argument
check, the host engine, the agent's flags, decision log, gate and series, and the tracker's host side as a
stand-alone program under the host sanitizers. The device tracker against this oracle: test_errsli_gpu.py."""

import io
import json
import os

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.collector import otlp
from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.contracts import semconv
from llm_slo_ebpf_toolkit_amd.pipeline import errsli as es
from llm_slo_ebpf_toolkit_amd.signals.metadata import Interner
from tests import errsli_scenarios as sc

T0 = 1_700_000_000_000_000_000
RES = {"service.name": "rag-service", "k8s.pod.uid": "pod-a"}
OK, CLIENT, CANCELLED, THROTTLED, TIMEOUT, UNAVAILABLE, SERVER, OTHER = range(8)


# ---- the field and the classification -----------------------------------------------------------------

def test_the_outcome_field_of_the_flags_word():
    assert (R.SPAN_OUTCOME_SHIFT, R.SPAN_OUTCOME_MASK) == (4, 0xF0) and es.CLASSES[SERVER] == "server" and len(es.CLASSES) == 8
    for c in range(16):
        assert R.pack_outcome(c) == c << 4 and R.span_outcome(0xFFFFFF0F | R.pack_outcome(c)) == c
    a = np.arange(16)
    assert R.pack_outcome(a).dtype == np.uint32 and R.span_outcome(R.pack_outcome(a) | np.uint32(0xFFFFFF0F)).tolist() == a.tolist()
    assert R.span_outcome(np.array([0xFFFFFF0F], np.uint32)).tolist() == [0]
    for bad in (-1, 16):
        with pytest.raises(ValueError):
            R.pack_outcome(bad)
        with pytest.raises(ValueError):
            R.pack_outcome(np.array([0, bad]))
    assert R.SPAN_OUTCOME_MASK & (R.SPAN_LATE | R.SPAN_NO_SLI | R.SPAN_FIRST_TOKEN | R.SPAN_START) == 0
    assert R.SPAN_OUTCOME_MASK & int(R.pack_tpot_us(R.SPAN_TPOT_MAX)) == 0
    assert semconv.ATTR_SLO_ERROR == "llm.slo.error"


HTTP = {429: THROTTLED, 408: TIMEOUT, 504: TIMEOUT, 499: CANCELLED, 502: UNAVAILABLE, 503: UNAVAILABLE, 500: SERVER, 501: SERVER,
        505: SERVER, 599: SERVER, 400: CLIENT, 401: CLIENT, 403: CLIENT, 404: CLIENT, 422: CLIENT, 498: CLIENT, 200: OK, 204: OK,
        302: OK, 399: OK, 100: OK, 600: OK, 0: OK}
GRPC = {0: OK, 1: CANCELLED, 4: TIMEOUT, 8: THROTTLED, 14: UNAVAILABLE, 2: SERVER, 10: SERVER, 12: SERVER, 13: SERVER, 15: SERVER,
        3: CLIENT, 5: CLIENT, 6: CLIENT, 7: CLIENT, 9: CLIENT, 11: CLIENT, 16: CLIENT, 17: OK, -1: OK}


def test_outcome_class_every_code_every_rule_the_precedence_and_garbage():
    oc = otlp.outcome_class
    for code, want in HTTP.items():
        assert oc({"http.response.status_code": code}) == want, code
        assert oc({"http.status_code": code}) == want, code
        assert oc({"http.response.status_code": str(code)}) == want and oc({"http.response.status_code": float(code)}) == want
    assert oc({"http.response.status_code": 503, "http.status_code": 429}) == UNAVAILABLE, "the new key first"
    for code, want in GRPC.items():
        assert oc({"rpc.grpc.status_code": code}) == want, code
    for text, want in (("CancelledError", CANCELLED), ("client_cancel", CANCELLED), ("TimeoutError", TIMEOUT),
                       ("DEADLINE_EXCEEDED", TIMEOUT), ("Throttled", THROTTLED), ("rate_limit_exceeded", THROTTLED),
                       ("RateLimitError", THROTTLED), ("java.io.IOException", OTHER), ("x", OTHER), ("", OK),
                       ("cancel_after_timeout", CANCELLED)):
        assert oc({"error.type": text}) == want, text
    assert oc({}, 2) == OTHER and oc({}, 1) == OK and oc({}, 0) == OK and oc({}, None) == OK and oc({}) == OK
    for v, want in ((True, OTHER), ("true", OTHER), (1, OTHER), (False, OK), ("no", OK), (0, OK)):
        assert oc({semconv.ATTR_SLO_ERROR: v}) == want, v
    # the first source that yields a class decides; one that yields nothing passes on
    assert oc({"http.response.status_code": 429, "rpc.grpc.status_code": 13, "error.type": "timeout"}, 2) == THROTTLED
    assert oc({"http.response.status_code": 200, "rpc.grpc.status_code": 13, "error.type": "timeout"}, 2) == SERVER
    assert oc({"http.response.status_code": 200, "rpc.grpc.status_code": 0, "error.type": "timeout"}, 2) == TIMEOUT
    assert oc({"http.response.status_code": 200, "rpc.grpc.status_code": 0}, 2) == OTHER
    assert oc({"http.response.status_code": 200, "rpc.grpc.status_code": 0, semconv.ATTR_SLO_ERROR: True}, 1) == OTHER
    # a value that is not a number where one is expected yields nothing
    for junk in ("abc", "", None, True, [503], {"a": 1}, float("nan"), float("inf"), 503.5, b"503"):
        assert oc({"http.response.status_code": junk}) == OK, junk
        assert oc({"rpc.grpc.status_code": junk}) == OK, junk
        assert oc({"http.response.status_code": junk, "rpc.grpc.status_code": 14}) == UNAVAILABLE
        assert oc({}, junk) == OK, junk
    assert oc({"error.type": 5}) == OK and oc({"error.type": None}) == OK and oc({"error.type": True}, 2) == OTHER
    assert oc({"http.response.status_code": None, "http.status_code": 504}) == TIMEOUT


def _vi(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def _ld(fn, payload):
    return _vi((fn << 3) | 2) + _vi(len(payload)) + payload


def _proto_span(status=None, attrs=()):
    """One request span, encoded by hand: Span fields 1, 2, 7, 8, 9 and, with ``status``, 15 = Status."""
    sp = _ld(1, bytes(range(16))) + _ld(2, bytes(range(8)))
    sp += _vi((7 << 3) | 1) + T0.to_bytes(8, "little") + _vi((8 << 3) | 1) + (T0 + 20_000_000).to_bytes(8, "little")
    for k, v in attrs:
        sp += _ld(9, _ld(1, k.encode()) + _ld(2, _vi((3 << 3) | 0) + _vi(v)))
    if status is not None:
        sp += _ld(15, status)
    res = _ld(1, _ld(1, _ld(1, b"service.name") + _ld(2, _ld(1, b"rag-service"))))
    return _ld(1, res + _ld(2, _ld(2, sp)))


def test_the_span_status_through_parse_proto_with_a_hand_encoded_field_15():
    err = _ld(2, b"upstream reset") + _vi((3 << 3) | 0) + _vi(2)   # message, then code = ERROR
    for status, want in ((err, 2), (_vi((3 << 3) | 0) + _vi(1), 1), (_vi((3 << 3) | 0) + _vi(0), 0), (_ld(2, b"only a message"), None),
                         (b"", None), (None, None)):
        (_res, d), = otlp.parse_proto(_proto_span(status))
        assert d.get("statusCode") == want, (status, d)
    (_res, d), = otlp.parse_proto(_proto_span(err, [("http.response.status_code", 503)]))
    assert d["statusCode"] == 2 and d["attrs"] == {"http.response.status_code": 503} and d["startTimeUnixNano"] == T0
    m = otlp.SpanMapper(otlp.GroupTable(4), Interner().id, error_sli=True)
    r = m.records(otlp.parse_proto(_proto_span(err)))
    assert len(r) == 1 and int(r["flags"][0]) == R.pack_outcome(OTHER) and np.isnan(r["ttft_ms"][0])
    r = m.records(otlp.parse_proto(_proto_span(err, [("http.response.status_code", 503)])))
    assert int(r["flags"][0]) == R.pack_outcome(UNAVAILABLE)


def _json(spans):
    """[(trace id, span id, parent, t0, t1, attrs, status or None)] as an OTLP/JSON export."""
    def av(v):
        if isinstance(v, bool):
            return {"boolValue": v}
        if isinstance(v, float):
            return {"doubleValue": v}
        return {"intValue": str(v)} if isinstance(v, int) else {"stringValue": v}

    return json.dumps({"resourceSpans": [{
        "resource": {"attributes": [{"key": k, "value": av(v)} for k, v in RES.items()]},
        "scopeSpans": [{"scope": {"name": "s"}, "spans": [
            {"traceId": t, "spanId": s, **({"parentSpanId": p} if p else {}), "name": "x", "kind": 2,
             "startTimeUnixNano": str(t0), "endTimeUnixNano": str(t1),
             "attributes": [{"key": k, "value": av(v)} for k, v in a.items()], **({"status": st} if st is not None else {})}
            for t, s, p, t0, t1, a, st in spans]}]}]}).encode()


def _tid(i):
    return f"{i:032x}"


def _final(i, ttft=None, status=None, **attrs):
    return (_tid(i), "00000000000000a1", "", T0, T0 + 20_000_000, {**({"llm.slo.ttft_ms": ttft} if ttft is not None else {}), **attrs},
            status)


def test_the_span_status_through_parse_json_as_an_integer_and_by_name():
    for code, want in ((2, 2), (1, 1), (0, 0), ("STATUS_CODE_ERROR", 2), ("STATUS_CODE_OK", 1), ("STATUS_CODE_UNSET", 0), ("2", 2),
                       ("nonsense", 0), (None, None), ([], 0)):
        (_res, d), = otlp.parse_json(_json([_final(1, status={"code": code, "message": "m"})]))
        assert d.get("statusCode") == want, code
    for st in (None, {}, {"message": "no code"}):
        (_res, d), = otlp.parse_json(_json([_final(1, status=st)]))
        assert "statusCode" not in d
    m = otlp.SpanMapper(otlp.GroupTable(4), Interner().id, error_sli=True)
    for code in (2, "STATUS_CODE_ERROR"):
        r = m.records(otlp.parse_json(_json([_final(1, status={"code": code})])))
        assert int(r["flags"][0]) == R.pack_outcome(OTHER)


# ---- the mapper ---------------------------------------------------------------------------------------

def _mapper(**kw):
    return otlp.SpanMapper(otlp.GroupTable(4), Interner().id, **kw)


def test_the_mapper_off_is_the_mapper_of_today_and_on_only_bits_4_to_7_of_finishing_records_differ():
    h = "http.response.status_code"
    start = (_tid(1), "00000000000000c1", "", T0, T0, {"llm.slo.request_start": True, h: 503}, {"code": 2})
    early = (_tid(1), "00000000000000f1", "00000000000000a1", T0, T0 + 9_000_000, {"llm.slo.ttft_ms": 9.0, "llm.slo.ttft_early": True,
                                                                                 h: 503}, {"code": 2})
    batch = [start, early, _final(1, 9.5, **{h: 200}), _final(2, 15.0, **{h: 429}), _final(3, None, {"code": 2}, **{h: 503}),
             _final(4, None, None, **{"rpc.grpc.status_code": 4}), _final(5, 12.0, {"code": 2}), _final(6, 12.0)]
    plain, off, on = _mapper(), _mapper(error_sli=False), _mapper(error_sli=True)
    for m in (plain, off, on):
        m.slo_ms, m.late_before_ns = 1.0, T0 + 50_000_000  # every record is late as well
    a, b, c = (m.records(otlp.parse_json(_json(batch))) for m in (plain, off, on))
    assert len(a) == 8 and a.tobytes() == b.tobytes()
    assert a["flags"].tolist() == [R.SPAN_START | R.SPAN_NO_SLI, R.SPAN_FIRST_TOKEN | R.SPAN_LATE, R.SPAN_NO_SLI | R.SPAN_LATE] + \
        [R.SPAN_LATE] * 5
    masked = c.copy()
    masked["flags"] &= np.uint32(~R.SPAN_OUTCOME_MASK & 0xFFFFFFFF)
    assert masked.tobytes() == a.tobytes(), "only bits 4-7 differ"
    # the start and the first-token record carry nothing, whatever their attributes say; a failed root span
    # without a TTFT (records 4 and 5) gets its class
    assert R.span_outcome(c["flags"]).tolist() == [0, 0, OK, THROTTLED, UNAVAILABLE, TIMEOUT, OTHER, OK]
    assert np.isnan(c["ttft_ms"][4]) and np.isnan(c["ttft_ms"][5]) and np.isnan(a["ttft_ms"][4])
    # decode_sli beside it: both fields, disjoint bits
    both = _mapper(error_sli=True, decode_sli=True).records(otlp.parse_json(_json([_final(9, 12.0, **{h: 500, "llm.slo.tpot_ms": 40.0})])))
    assert int(both["flags"][0]) == R.pack_outcome(SERVER) | R.pack_tpot_us(40_000)
    # through the tracker's rules: six finished requests, three of them against the budget
    o = es.ErrorSliOracle(**sc._cfg(group_cap=4))
    r = o.results(o.step_records(c, 4), 4)
    assert r["counts"][0].tolist() == [2, 0, 0, 1, 1, 1, 0, 1] and es.stats_dict(r["stats"])["observed"] == 6
    r = o.results(o.step_records(a, 4), 4)
    assert r["counts"][0].tolist() == [6, 0, 0, 0, 0, 0, 0, 0], "switched off every finished request is ok"


def test_the_demo_service_s_failing_request_yields_class_server():
    from llm_slo_ebpf_toolkit_amd.demo import rag_service as rs

    class Boom(rs.StubBackend):
        def generate(self, *a, **k):
            raise RuntimeError("backend down")

    got = []
    for backend in (rs.StubBackend(), Boom()):
        svc = rs.RagService(backend, otlp_endpoint="")
        svc.spans.add = lambda spans, urgent=False: got.extend(spans)
        try:
            svc.chat({"prompt": "why is ttft high", "profile": "chat_short", "max_tokens": 3, "request_id": f"r-{len(got)}"})
        except RuntimeError:
            pass
    body = json.dumps({"resourceSpans": [{"resource": {"attributes": [{"key": "service.name", "value": {"stringValue": "rag-service"}}]},
                                          "scopeSpans": [{"spans": got}]}]}).encode()
    parsed = otlp.parse_json(body)
    roots = [d for _r, d in parsed if d["name"] == "chat.request"]
    assert len(roots) == 2 and [d.get("statusCode") for d in roots] == [None, 2]
    assert [d["attrs"]["http.response.status_code"] for d in roots] == [200, 500] and rs.RagService.FAIL_STATUS == 500
    recs = _mapper(error_sli=True).records(parsed)
    fin = recs[(recs["flags"] & (R.SPAN_START | R.SPAN_FIRST_TOKEN)) == 0]
    assert R.span_outcome(fin["flags"]).tolist() == [OK, SERVER] and np.isnan(fin["ttft_ms"][1])


# ---- the mask-only claim ------------------------------------------------------------------------------

def test_the_seven_other_oracles_and_the_host_engine_read_the_flag_bits_by_mask():
    from llm_slo_ebpf_toolkit_amd.pipeline.decodesli import DecodeSliOracle
    from llm_slo_ebpf_toolkit_amd.pipeline.drift import DriftOracle
    from llm_slo_ebpf_toolkit_amd.pipeline.exemplars import EXEMPLAR, ExemplarOracle
    from llm_slo_ebpf_toolkit_amd.pipeline.onset import OnsetOracle
    from llm_slo_ebpf_toolkit_amd.pipeline.openreq import OpenRequestOracle
    from llm_slo_ebpf_toolkit_amd.pipeline.podrank import PodRankOracle
    from llm_slo_ebpf_toolkit_amd.pipeline.slisketch import SliSketchOracle
    from tests.onset_scenarios import BIN, Q0, cut_of, edge_window

    rng = np.random.default_rng(5)
    G, q = 3, Q0 + 50
    plain = edge_window(rng, 200, G, q, 64)
    plain["trace_h"] = np.arange(1, len(plain) + 1, dtype=np.uint64)  # one record a trace: the open requests are ordered
    plain["pod_id"] = rng.integers(1, 9, len(plain))
    plain["flags"] |= R.pack_tpot_us(rng.integers(1, 200_000, len(plain)))
    # the window's records are first-token records; every other one becomes the record that ends its request
    plain["flags"][::2] &= np.uint32(~R.SPAN_FIRST_TOKEN & 0xFFFFFFFF)
    finishing = (plain["flags"] & (R.SPAN_START | R.SPAN_FIRST_TOKEN)) == 0
    packed = plain.copy()
    packed["flags"] |= np.where(finishing, R.pack_outcome(rng.integers(1, 8, len(plain))), 0).astype(np.uint32)
    assert finishing.sum() > 100 and (packed["flags"][finishing] != plain["flags"][finishing]).all()
    assert ((packed["flags"] ^ plain["flags"]) & np.uint32(~R.SPAN_OUTCOME_MASK & 0xFFFFFFFF) == 0).all()
    cut = cut_of(q)
    made = (lambda: OpenRequestOracle(cap=1 << 10, span_cap=1024, group_cap=G, slo_ms=800.0),
            lambda: SliSketchOracle(span_cap=1024, group_cap=G, windows=2),
            lambda: ExemplarOracle(k=3, windows=2, span_cap=1024, group_cap=G),
            lambda: PodRankOracle(k=3, windows=2, pair_cap=64, span_cap=1024, group_cap=G, slo_ms=800.0),
            lambda: OnsetOracle(bins=64, bin_ns=BIN, ref_ppm=250_000, alarm=3, span_cap=1024, group_cap=G, slo_ms=800.0),
            lambda: DecodeSliOracle(span_cap=1024, group_cap=G, windows=2),
            lambda: DriftOracle(span_cap=1024, group_cap=G, recent=1, gap=1, baseline=2))
    args = ((cut, cut - 160_000_000, G), (G,), (G,), (G,), (cut, G), (G,), (G,))
    for make, extra in zip(made, args):
        out = []
        for recs in (plain, packed):
            o = make()
            out.append(o.results(o.step_records(recs, *extra), G))
        a, b = out
        assert set(a) == set(b)
        for key in a:
            x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
            if x.dtype == EXEMPLAR:
                # an exemplar row quotes its record's whole flags word, so it carries the class too, as it does the
                # TPOT: the same records are chosen, and the quoted word is the record's
                assert ((x["flags"] ^ y["flags"]) & np.uint32(~R.SPAN_OUTCOME_MASK & 0xFFFFFFFF) == 0).all()
                y = y.copy()
                y["flags"] = x["flags"]
            assert x.tobytes() == y.tobytes(), (type(o).__name__, key)
    # pipeline/cpu.py: the host engine's own results on the two windows
    ra, _ = sc.run_pipeline("cpu", [plain], G, 0)
    rb, _ = sc.run_pipeline("cpu", [packed], G, 0)
    assert set(ra[0]) == set(rb[0])
    for key in ra[0]:
        assert np.ascontiguousarray(ra[0][key]).tobytes() == np.ascontiguousarray(rb[0][key]).tobytes(), key


# ---- the oracle ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_oracle_equals_the_brute_force_after_every_step_and_the_hand_computed_expectation(name):
    c = sc.case(name)
    ref, brute, seen = es.ErrorSliOracle(**c.cfg), sc.Brute(**c.cfg), []
    assert ref.budget_ppm == brute.budget == sc.BUDGET
    for w, (recs, G) in enumerate(c.steps):
        i = ref.step_records(recs, G)
        a = ref.results(i, ref.group_cap)
        sc.same_results(a, brute.step(recs, G), f"{name} step {w}")
        sc.same_resident(ref.resident(), brute.resident(), f"{name} step {w}")
        blk, off = ref.block(i), es.layout(ref.group_cap)
        assert blk.dtype == np.uint32 and len(blk) == off["words"]
        assert blk[off["stats"]:off["stats"] + 8].tolist() == a["stats"].tolist()
        assert blk[off["firing"]:off["firing"] + ref.group_cap].tolist() == a["firing"].tolist()
        part = ref.results(i, G)
        assert all(len(part[k]) == G for k in es.RESULT_FIELDS if k != "stats")
        seen.append(a)
    if c.check is not None:
        c.check(seen)


def test_the_budget_the_pairs_and_the_classes_as_the_agent_gives_them():
    assert [es.budget_ppm(t) for t in (0.999, 0.9, 0.99, 0.0, 0.9999999, 0.5, 0.9995)] == [1000, 100000, 10000, 10 ** 6, 1, 500000, 500]
    assert es.parse_pairs(es.DEFAULT_PAIRS_S, 1000.0) == [(3600, 300, 14400), (21600, 1800, 6000)]
    assert es.parse_pairs("3600:300:14.4", 2000.0) == [(1800, 150, 14400)]
    assert es.parse_pairs("1:0.1:2", 300.0) == [(4, 1, 2000)], "ceil, at least 1"
    with pytest.raises(ValueError, match="21600:1800:6.*43200 windows"):
        es.parse_pairs(es.DEFAULT_PAIRS_S, 500.0)
    for bad in ("", "a:b:c", "10:5", "10:20:1", "10:5:0", "0:0:1", "10:5:nan", "1:1:1,1:1:1,1:1:1,1:1:1,1:1:1"):
        with pytest.raises(ValueError):
            es.parse_pairs(bad, 1000.0)
    assert es.bad_mask_of(es.DEFAULT_BAD_CLASSES) == es.BAD_DEFAULT == 0xF8
    assert es.bad_mask_of("server") == 0x40 and es.bad_mask_of(" Client , cancelled,") == 0x06
    for bad in ("ok", "nonsense", "", ","):
        with pytest.raises(ValueError):
            es.bad_mask_of(bad)
    top = (1 << 32) - 1
    assert es.burns(top, top, top, 10 ** 9) and not es.burns(top, top - 1, 0, 10 ** 9) and not es.burns(0, 0, 0, 1)


def test_every_configuration_check_and_every_refused_step():
    for kw in sc.BAD_CONFIGS:
        with pytest.raises(ValueError, match="error sli"):
            es.ErrorSliOracle(**kw)
    for kw in sc.GOOD_CONFIGS:
        es.ErrorSliOracle(**kw)
    o = es.ErrorSliOracle(**sc._cfg(span_cap=8))
    recs = np.ascontiguousarray(sc.of(0, ok=5, server=3))
    a = recs.ctypes.data
    o.step_records(recs, 3)
    before = {k: np.array(v, copy=True) for k, v in o.resident().items()}
    for bad in (lambda: o.step([(a, 63)], 3), lambda: o.step_records(recs[:1], 4), lambda: o.step_records(recs[:1], -1),
                lambda: o.step_records(np.concatenate([recs, recs[:1]]), 3), lambda: o.step([(0, 64)], 3),
                lambda: o.step([(a, 8 * 64), (a, 64)], 3)):
        with pytest.raises(ValueError, match="error sli step"):
            bad()
    sc.same_resident(o.resident(), before, "a refused step changes nothing")
    i = o.step([(a, 4 * 64), (a, 0), (0, 0), (a + 4 * 64, 4 * 64)], 3)
    assert i == 1 and o.results(i, 3)["counts_roll"][0].tolist() == [10, 0, 0, 0, 0, 0, 6, 0]
    with pytest.raises(IndexError):
        o.results(-1, 3)
    with pytest.raises(IndexError):
        o.results(i - 3, 3)
    with pytest.raises(ValueError):
        o.results(i, 4)


# ---- the pipeline -------------------------------------------------------------------------------------

def test_pipeline_on_the_host_engine_carries_the_new_keys_only_when_switched_on():
    from llm_slo_ebpf_toolkit_amd.pipeline.window import WindowPipeline

    rng = np.random.default_rng(47)
    groups = [3, 3, 2, 3]
    wins = [sc.mixed_window(rng, 40, 3, p_bad=0.3) if w != 2 else np.zeros(0, R.SPAN) for w in range(4)]
    off, none = sc.run_pipeline("cpu", wins, groups, 0)
    onr, err = sc.run_pipeline("cpu", wins, groups, 2)
    ref = es.ErrorSliOracle(span_cap=1024, group_cap=8, windows=2, target=sc.TARGET, pairs=sc.PIPE_PAIRS, min_requests=5)
    assert none == []
    for w, (a, b, d) in enumerate(zip(off, onr, err)):
        assert not set(a) & set(es.RESULT_KEYS) and set(b) == set(a) | set(es.RESULT_KEYS)
        for key in a:
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"window {w} {key}")
        want = ref.results(ref.step_records(wins[w], groups[w]), groups[w])
        sc.same_results(d, want, f"window {w}")
        for key, v in es.result_keys(want).items():
            np.testing.assert_array_equal(b[key], v, err_msg=f"window {w} {key}")
    assert int(onr[2]["err_counts"].sum()) == 0 and int(onr[2]["err_counts_roll"].sum()) > 0
    with pytest.raises(ValueError, match="one GPU: no communicator, no sharding"):
        WindowPipeline(1024, 64, 4, engine="cpu", shard=(0, 2), error_sli=2)
    with pytest.raises(ValueError, match="error sli: target"):
        WindowPipeline(1024, 64, 4, engine="cpu", error_sli=2, error_target=1.0)
    with pytest.raises(ValueError, match="error sli: windows"):
        WindowPipeline(1024, 64, 4, engine="cpu", error_sli=40000)
    with pytest.raises(ValueError, match="error sli: a pair"):
        WindowPipeline(1024, 64, 4, engine="cpu", error_sli=2, error_pairs=[(3, 1, 1000)])
    p = WindowPipeline(1024, 64, 4, engine="cpu")
    try:
        assert p.errors is None and p._no_side_tracker
    finally:
        p.close()
    p = WindowPipeline(1024, 64, 4, engine="cpu", error_sli=24)
    try:
        assert p.errors.pairs == [(24, 2, 14400)] and not p._no_side_tracker and not p.copy_ahead
    finally:
        p.close()


# ---- the agent ----------------------------------------------------------------------------------------

def _agent(tmp_path, tag, **kw):
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions

    log = tmp_path / f"decisions-{tag}.jsonl"
    o = AgentOptions(engine="cpu", source="replay", gpus=1, window_events=2048, window_spans=128, window_groups=8,
                     window_ms=300, metrics_bind="", output="stdout", ring_name=f"/mislo-es-{tag}-{os.getpid()}",
                     config="", min_confidence=0.0, scenario="full", disable_overhead_guard=True,
                     decision_log=str(log), **kw)
    out = io.StringIO()
    a = Agent(o, out_stream=out)
    try:
        assert a.run_windows(max_windows=4) == 0
    finally:
        a.close()
    return a, [json.loads(ln) for ln in log.read_text().splitlines()], out.getvalue()


def test_agent_flags_defaults_and_what_is_refused():
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions
    from llm_slo_ebpf_toolkit_amd.cli.agent import parse

    o, _ = parse(["--engine", "cpu", "--error-sli", "--error-slo-target", "0.99", "--error-burn-pairs", "600:60:10,60:5:20",
                  "--error-min-requests", "7", "--error-bad-classes", "server,timeout", "--error-horizon-windows", "900",
                  "--emit-on-error-burn"])
    assert (o.error_sli, o.error_slo_target, o.error_burn_pairs, o.error_min_requests, o.error_bad_classes, o.error_horizon_windows,
            o.emit_on_error_burn) == (True, 0.99, "600:60:10,60:5:20", 7, "server,timeout", 900, True)
    d = parse([])[0]
    assert (d.error_sli, d.error_slo_target, d.error_burn_pairs, d.error_min_requests, d.error_bad_classes, d.error_horizon_windows,
            d.emit_on_error_burn) == (False, 0.999, es.DEFAULT_PAIRS_S, 20, es.DEFAULT_BAD_CLASSES, 0, False)
    assert AgentOptions().error_sli is False and AgentOptions().emit_on_error_burn is False
    kw = dict(engine="cpu", source="replay", config="", output="stdout", metrics_bind="")
    a = Agent(AgentOptions(ring_name=f"/mislo-es2-{os.getpid()}", window_ms=2000, **kw))
    try:
        assert a.error_pairs() == [(1800, 150, 14400), (10800, 900, 6000)] and a.error_horizon() == 10800
        assert a.error_bad_mask() == 0xF8
    finally:
        a.close()
    a = Agent(AgentOptions(ring_name=f"/mislo-es3-{os.getpid()}", window_ms=2000, error_horizon_windows=12000, **kw))
    try:
        assert a.error_horizon() == 12000
    finally:
        a.close()
    for extra, match in ((dict(gpus=2, error_sli=True), "--error-sli runs on one GPU"),
                         (dict(emit_on_error_burn=True), "--emit-on-error-burn needs --error-sli"),
                         (dict(error_sli=True, window_ms=500), "21600:1800:6.*43200 windows"),
                         (dict(error_sli=True, error_bad_classes="ok"), "no class that can burn")):
        a = Agent(AgentOptions(ring_name=f"/mislo-es4-{os.getpid()}", **{**kw, **extra}))
        try:
            with pytest.raises(ValueError, match=match):
                a.run_windows(max_windows=1)
        finally:
            a.close()


PAIRS = [(3, 1, 1000)]


def _fabricated():
    """Service 1 ("chat") over two steps of the both-windows case: 10 ok, then 8 ok + 2 server."""
    o = es.ErrorSliOracle(**sc._cfg(windows=3, pairs=PAIRS))
    o.step_records(sc.of(1, ok=10), 3)
    i = o.step_records(sc.cat(sc.of(1, ok=8, server=2), sc.of(2, client=1)), 3)
    return es.result_keys(o.results(i, 3)), o


def test_the_decision_log_entry_and_the_series_from_a_fabricated_result():
    from llm_slo_ebpf_toolkit_amd.agent.metrics import AgentMetrics
    from llm_slo_ebpf_toolkit_amd.export.prometheus import parse_exposition

    res, o = _fabricated()
    e = [es.summary(res, g, PAIRS, o.budget_ppm, o.bad_mask) for g in range(3)]
    keys = {"requests", "bad", "ratio", "by_class"}
    assert all(set(x) == keys | {"horizon", "burn", "firing", "age_windows"} and set(x["horizon"]) == keys for x in e)
    none = {"requests": 0, "bad": 0, "ratio": None, "by_class": dict.fromkeys(es.CLASSES, 0)}
    assert e[0] == {**none, "horizon": none, "firing": 0, "age_windows": 0,
                    "burn": [{"long_windows": 3, "short_windows": 1, "factor": 1.0, "long": None, "short": None, "firing": False}]}
    assert e[1]["requests"] == 10 and e[1]["bad"] == 2 and e[1]["ratio"] == 0.2 and e[1]["by_class"]["server"] == 2
    assert e[1]["horizon"]["requests"] == 20 and e[1]["horizon"]["ratio"] == 0.1 and e[1]["horizon"]["by_class"]["ok"] == 18
    # burn rates on the host from the sums: 2/20 and 2/10 over a 10 % budget
    assert e[1]["burn"] == [{"long_windows": 3, "short_windows": 1, "factor": 1.0, "long": 1.0, "short": 2.0, "firing": True}]
    assert e[1]["firing"] == 1 and e[1]["age_windows"] == 1
    assert e[2]["requests"] == 1 and e[2]["bad"] == 0 and e[2]["ratio"] == 0.0 and e[2]["burn"][0]["long"] == 0.0 and e[2]["firing"] == 0
    json.dumps(e)
    m = AgentMetrics("probe", "auto", [], [])
    stats = {"observed": 11, "out_of_group": 2, "reserved": 3}
    for _ in range(2):
        m.observe_errors(res, stats, ["rag", "chat"], PAIRS, o.budget_ppm, o.bad_mask)
    text = m.registry.exposition()
    v = parse_exposition(text)
    assert v['llm_slo_agent_request_outcomes_total{service="chat",outcome="ok"}'] == 16
    assert v['llm_slo_agent_request_outcomes_total{service="chat",outcome="server"}'] == 4
    assert v['llm_slo_agent_request_outcomes_total{service="group-2",outcome="client"}'] == 2
    assert 'outcome="timeout"' not in text and 'llm_slo_agent_request_outcomes_total{service="rag"' not in text
    assert v['llm_slo_agent_error_ratio{service="chat"}'] == pytest.approx(0.1) and v['llm_slo_agent_error_ratio{service="group-2"}'] == 0
    assert 'llm_slo_agent_error_ratio{service="rag"}' not in text, "no request: no series"
    assert v['llm_slo_agent_error_burn_rate{service="chat",pair="3:1:1",window="long"}'] == pytest.approx(1.0)
    assert v['llm_slo_agent_error_burn_rate{service="chat",pair="3:1:1",window="short"}'] == pytest.approx(2.0)
    assert v['llm_slo_agent_error_burn_firing{service="chat",pair="3:1:1"}'] == 1
    assert v['llm_slo_agent_error_burn_firing{service="rag",pair="3:1:1"}'] == 0
    for reason in es.EVENT_STATS:
        assert v[f'llm_slo_agent_error_events_total{{reason="{reason}"}}'] == 2 * stats[reason]


@pytest.mark.timeout(120)
def test_the_agent_logs_an_errors_entry_per_scored_group_and_off_means_nothing_new(tmp_path):
    from llm_slo_ebpf_toolkit_amd.contracts import validator

    a, rows, out = _agent(tmp_path, "on", error_sli=True, error_burn_pairs="3:0.3:2", error_min_requests=1)
    assert rows and all("errors" in r and "gate" not in r for r in rows)
    assert a.specs[0].error_sli == 10 and a.specs[0].error_pairs == ((10, 1, 2000),) and a.specs[0].error_bad_mask == 0xF8
    assert a.mapper is None or a.mapper.error_sli
    emitted = [json.loads(ln) for ln in out.splitlines() if ln.startswith('{"incident_id"')]
    assert emitted
    for d in emitted:
        assert "errors" not in d
        validator.validate("incident-attribution", d)
    # the replay's spans carry class 0: every finished request is ok, nothing fires
    assert all(r["errors"]["bad"] == 0 and r["errors"]["firing"] == 0 and r["errors"]["age_windows"] == 0 for r in rows)
    assert any(r["errors"]["requests"] > 0 and r["errors"]["ratio"] == 0.0 for r in rows)
    text = a.metrics.registry.exposition()
    assert 'llm_slo_agent_request_outcomes_total{' in text and 'llm_slo_agent_error_events_total{reason="reserved"}' in text
    b, rows_off, out_off = _agent(tmp_path, "off")
    assert b.specs[0].error_sli == 0 and all("errors" not in r and "gate" not in r for r in rows_off)
    assert "llm_slo_agent_request_outcomes_total{" not in b.metrics.registry.exposition()
    assert "llm_slo_agent_error_events_total{" not in b.metrics.registry.exposition()
    # the replay is cut by the wall clock, so two runs need not see the same windows: the shapes are compared
    off = [json.loads(ln) for ln in out_off.splitlines() if ln.startswith('{"incident_id"')]
    assert off and {frozenset(d) for d in off} == {frozenset(d) for d in emitted}, "emitted incidents keep their fields"
    assert {frozenset(r) | {"errors"} for r in rows_off} == {frozenset(r) for r in rows}


# ---- the gate -----------------------------------------------------------------------------------------

CALM, FAILING, AFTER = 6, 5, 4


def _phase_stream():
    """One service, 30 requests a window, every one with a TTFT of 100-300 ms (no TTFT breach anywhere): calm
    windows, then a failing phase in which a third of the requests are answered 503 at once, then calm again."""
    rng = np.random.default_rng(8)
    wins = []
    for w in range(CALM + FAILING + AFTER):
        failing = CALM <= w < CALM + FAILING
        cls = np.where((np.arange(30) % 3 == 0) & failing, UNAVAILABLE, OK)
        r = sc.recs(cls, [0] * 30, 0, rng.uniform(100.0, 300.0, 30))
        r["ts_ns"] = T0 + w * 160_000_000 + np.arange(30)
        r["trace_h"] = np.arange(1, 31, dtype=np.uint64) + np.uint64(1000 * w)
        wins.append(r)
    return wins


def _decisions(tmp_path, tag, results, **kw):
    """Every window's results through the agent's emission gate (Agent._attributions); the log's raw lines."""
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions

    log = tmp_path / f"gate-{tag}.jsonl"
    o = AgentOptions(engine="cpu", source="replay", gpus=1, window_ms=160, metrics_bind="", output="stdout", config="",
                     ring_name=f"/mislo-esg-{tag}-{os.getpid()}", min_confidence=0.0, decision_log=str(log), ttft_slo_ms=800.0,
                     error_slo_target=sc.TARGET, error_burn_pairs="0.32:0.16:1,0.32:0.32:2", error_min_requests=5, **kw)
    a = Agent(o, out_stream=io.StringIO())
    try:
        assert a.error_pairs() == [tuple(p) for p in sc.PIPE_PAIRS]
        model, _image, _meta = a._load_model()
        incidents = [a._attributions(1, ["chat"], r, T0 + w * 160_000_000, model) for w, r in enumerate(results)]
    finally:
        a.close()
    return log.read_text().splitlines(), incidents


@pytest.mark.timeout(120)
def test_the_error_gate_opens_failing_windows_only_and_the_recovered_rule_steps_aside(tmp_path):
    """The phase stream through the host engine, every window's results through the agent's gate. No request
    breaches the TTFT SLO, so the burn gate never opens; every window completes 30 requests without a breach, so
    ``recovered`` (at its default, 2 requests at this window length) would hold back every one of them."""
    wins = _phase_stream()
    results, tracked = sc.run_pipeline("cpu", wins, 1, 2, group_cap=2)
    plain, _ = sc.run_pipeline("cpu", wins, 1, 0, group_cap=2)
    t = lambda w: T0 + w * 160_000_000  # noqa: E731
    failing = {t(w) for w in range(CALM, CALM + FAILING)}
    # the tracker: a window with 10 of 30 against a 10 % budget burns both pairs; the window after the phase still
    # holds the last failing window in its two-window sums (10 of 60: pair 0's long burns, its short does not;
    # pair 1 at factor 2 needs 0.2 and has 0.167)
    assert [int(r["firing"][0]) for r in tracked] == [0] * CALM + [1] + [3] * (FAILING - 1) + [0] * AFTER
    assert [int(r["age"][0]) for r in tracked] == [0] * CALM + list(range(1, FAILING + 1)) + [0] * AFTER
    raw_on, inc_on = _decisions(tmp_path, "on", results, error_sli=True, emit_on_error_burn=True)
    on = [json.loads(x) for x in raw_on]
    assert len(on) == len(wins) and all("errors" in r for r in on)
    gated = [r for r in on if r.get("gate") == "errors"]
    assert {r["t_ns"] for r in gated} == failing, "the error gate opens in failing windows, and only there"
    assert all(r["emitted"] and r["why"] == "emitted" and r["breaches"] == 0 and r["requests"] == 30 for r in gated)
    assert all(r["errors"]["bad"] == 10 and r["errors"]["by_class"]["unavailable"] == 10 and r["errors"]["firing"] for r in gated)
    assert [r["errors"]["age_windows"] for r in gated] == list(range(1, FAILING + 1))
    assert gated[1]["errors"]["burn"][0] == {"long_windows": 2, "short_windows": 1, "factor": 1.0, "long": round(20 / 60 / 0.1, 6),
                                             "short": round(10 / 30 / 0.1, 6), "firing": True}
    assert all("gate" not in r and not r["emitted"] for r in on if r["t_ns"] not in failing)
    assert sum(len(x) for x in inc_on) == FAILING
    # the tracker on, the gate flag off: the same entries, nothing emitted, no gate key
    raw_log, inc_log = _decisions(tmp_path, "log", results, error_sli=True)
    log = [json.loads(x) for x in raw_log]
    assert all("gate" not in r and not r["emitted"] for r in log) and sum(len(x) for x in inc_log) == 0
    assert [r["errors"] for r in log] == [r["errors"] for r in on]
    # where the error gate opened the window but the window itself holds no failure, recovered applies as today:
    # the last failing window's sums, carried into a clean window by a pair that still fires
    carried = {k: np.array(v, copy=True) for k, v in results[CALM + FAILING].items()}
    carried["err_firing"] = np.array([1], np.uint32)
    raw_c, inc_c = _decisions(tmp_path, "carried", [carried], error_sli=True, emit_on_error_burn=True)
    row = json.loads(raw_c[0])
    assert row["errors"]["bad"] == 0 and row["errors"]["firing"] == 1 and not row["emitted"] and row["why"] == "recovered"
    assert "gate" not in row and inc_c == [[]]
    # with the flags off the log is byte for byte the one the same windows give without the tracker
    raw_off, inc_off = _decisions(tmp_path, "off", plain)
    stripped = [{k: v for k, v in r.items() if not k.startswith("err_")} for r in results]
    raw_stripped, _ = _decisions(tmp_path, "stripped", stripped)
    assert raw_off == raw_stripped and all("errors" not in x and "gate" not in x for x in raw_off)
    assert sum(len(x) for x in inc_off) == 0
    for a, b in zip(raw_off, raw_log):   # and the tracker adds its entry and nothing else
        ra, rb = json.loads(a), json.loads(b)
        assert {k: v for k, v in rb.items() if k != "errors"} == ra and list(rb)[-1] == "why"


# ---- the tracker's host side under the host sanitizers ------------------------------------------------

def test_errsli_host_side_under_address_and_ub_sanitizers(tmp_path):
    """ops/csrc/errsli_host.h (the class field, the burn compare against unsigned __int128 at the bounds, the
    budget, argument checks, layout, ranges) needs no device: a stand-alone program over it, built with
    AddressSanitizer + UBSan, run as a child process. It prints the layout of several group counts, which must be
    the Python mirror's."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "llm_slo_ebpf_toolkit_amd", "ops", "csrc")
    exe = tmp_path / "errsli_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-Wall", "-Werror", f"-I{csrc}", os.path.join(root, "tests", "native", "errsli_host_check.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "errsli host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
    got = [tuple(int(x) for x in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("layout ")]
    assert len(got) == 7
    for g, *at in got:
        off = es.layout(g)
        assert at == [off[k] for k in ("counts", "counts_roll", "pair_sums", "firing", "age", "stats", "words")]
    dev, = [int(ln.split()[1]) for ln in r.stdout.splitlines() if ln.startswith("device_bytes ")]
    assert dev == es.device_bytes(16384, 64, 3600)
