"""OTLP/HTTP trace receiver feeding the agent's span ring (VERDICT r1 missing #2).

REF enriches spans inside the OpenTelemetry collector: the `ebpfcorrelator` processor
(REF pkg/otel/processor/ebpfcorrelator/processor.go:29-49) sees every span of the RAG
service's request path (REF demo/rag-service/main.go:408-441) and joins it with eBPF signals
on the host. Here the join runs on the GPU, so the agent itself accepts the services' spans:

    POST /v1/traces   application/json (OTLP/JSON) or application/x-protobuf (OTLP/proto)

Each request's server span (a root span, or any span carrying the TTFT SLI attribute) becomes
one 64-byte SPAN record (collector/records.py SPAN) pushed into the span ring the window
engine DMAs from, with its identities mapped onto the ids the kernel side uses:

* trace id  -> ``trace_hash`` (low 64 bits of the W3C trace id; the GPU translates it through
  the kernel's trace definitions, ops/csrc/decode.hip k_decode_spans);
* pod       -> the agent's pod id for ``k8s.pod.uid`` (the same interner that fills the
  probes' cgroup -> pod map, collector/bpf.py discover_pods), else ``k8s.pod.name``;
* pid       -> ``process.pid``; connection -> (client port, server port, server IPv4) hashed
  like the probes' connection key (records.conn_hash);
* incident group -> ``service.name`` (one group per service, ``GroupTable``);
* SLI       -> ``llm.slo.ttft_ms`` (contracts/semconv.py) and the span duration;
* retrieval -> ``retr_ms``: the request's ``llm.slo.retrieval.{vectordb,network,dns}_ms`` summed over
  the spans of its trace (REF puts them on the ``chat.retrieval`` child span,
  demo/rag-service/main.go:393-397). The engine turns it into application evidence: the group's
  retrieval time beyond the kernel-attributed share (REF DecomposeRetrieval,
  pkg/otel/processor/ebpfcorrelator/correlator.go:179-194; models/bayes.py AppEvidence). A child
  span that arrives in an earlier export than its request span waits in a bounded table keyed by
  trace (an OTel SDK exports spans as they end: children first); one that arrives after its
  request span was pushed is not joined.

The protobuf decoder is a minimal wire-format walker over the OTLP trace messages
(ExportTraceServiceRequest / ResourceSpans / ScopeSpans / Span / KeyValue / AnyValue): no
generated code, no protobuf runtime.
"""

from __future__ import annotations

import collections
import http.server
import ipaddress
import json
import struct
import threading
from dataclasses import dataclass, field
from typing import Callable, Dict, Iterator, List, Optional, Tuple

import numpy as np

from ..contracts import semconv
from . import records

TTFT_KEYS = (semconv.ATTR_SLO_TTFT_MS, "gen_ai.server.time_to_first_token", "llm.ttft_ms")
RETRIEVAL_KEYS = (semconv.ATTR_RETRIEVAL_VECTORDB, semconv.ATTR_RETRIEVAL_NETWORK_MS, semconv.ATTR_RETRIEVAL_DNS_MS)


def retrieval_ms(attrs: Dict[str, object]) -> Optional[float]:
    """A span's application-reported retrieval time: its ``llm.slo.retrieval.*`` breakdown summed
    (None without one). Non-numeric, negative or non-finite parts are ignored."""
    tot, seen = 0.0, False
    for k in RETRIEVAL_KEYS:
        v = attrs.get(k)
        if v is None or isinstance(v, bool):
            continue
        try:
            f = float(v)
        except (TypeError, ValueError):
            continue
        if f >= 0.0 and f < float("inf"):
            tot += f
            seen = True
    return tot if seen else None


def trace_hash(trace_id) -> int:
    """Low 64 bits of a W3C trace id (hex string or 16 bytes); never 0 for a present id."""
    if not trace_id:
        return 0
    if isinstance(trace_id, (bytes, bytearray)):
        b = bytes(trace_id)[-8:]
        h = int.from_bytes(b, "big")
    else:
        s = str(trace_id).strip().lower()
        h = int(s[-16:], 16) if s else 0
    return h or 1


def trace_high_half(trace_id) -> Optional[int]:
    """High 64 bits of a 128-bit W3C trace id (hex string or 16 bytes); None for a shorter id."""
    try:
        if isinstance(trace_id, (bytes, bytearray)):
            b = bytes(trace_id)
            return int.from_bytes(b[-16:-8], "big") if len(b) >= 16 else None
        s = str(trace_id or "").strip().lower()
        return int(s[-32:-16], 16) if len(s) >= 32 else None
    except ValueError:
        return None


def span_hash(span_id) -> int:
    if not span_id:
        return 0
    if isinstance(span_id, (bytes, bytearray)):
        return int.from_bytes(bytes(span_id)[-8:], "big") or 1
    return int(str(span_id)[-16:], 16) or 1


# ---------------------------------------------------------------------------------------
# OTLP/proto wire walker
# ---------------------------------------------------------------------------------------

def _varint(b: bytes, i: int) -> Tuple[int, int]:
    v, shift = 0, 0
    while True:
        if i >= len(b):
            raise ValueError("truncated varint")
        c = b[i]
        i += 1
        v |= (c & 0x7F) << shift
        if not c & 0x80:
            return v, i
        shift += 7
        if shift > 63:
            raise ValueError("varint too long")


def _fields(b: bytes) -> Iterator[Tuple[int, int, object]]:
    """(field number, wire type, value) over one message's bytes."""
    i, n = 0, len(b)
    while i < n:
        key, i = _varint(b, i)
        fn, wt = key >> 3, key & 7
        if wt == 0:
            v, i = _varint(b, i)
        elif wt == 1:
            if i + 8 > n:
                raise ValueError("truncated fixed64")
            v = struct.unpack_from("<Q", b, i)[0]
            i += 8
        elif wt == 2:
            ln, i = _varint(b, i)
            if i + ln > n:
                raise ValueError("truncated bytes")
            v = b[i:i + ln]
            i += ln
        elif wt == 5:
            if i + 4 > n:
                raise ValueError("truncated fixed32")
            v = struct.unpack_from("<I", b, i)[0]
            i += 4
        else:
            raise ValueError(f"unsupported wire type {wt}")
        yield fn, wt, v


def _any_value(b: bytes):
    for fn, wt, v in _fields(b):
        if fn == 1:
            return bytes(v).decode("utf-8", "replace")
        if fn == 2:
            return bool(v)
        if fn == 3:
            return v - (1 << 64) if v >= 1 << 63 else v
        if fn == 4:
            return struct.unpack("<d", struct.pack("<Q", v))[0]
        if fn == 7:
            return bytes(v)
    return None


def _attrs_pb(items: List[bytes]) -> Dict[str, object]:
    out = {}
    for kv in items:
        k, val = "", None
        for fn, _wt, v in _fields(kv):
            if fn == 1:
                k = bytes(v).decode("utf-8", "replace")
            elif fn == 2:
                val = _any_value(v)
        if k:
            out[k] = val
    return out


def parse_proto(body: bytes) -> List[Tuple[Dict[str, object], dict]]:
    """ExportTraceServiceRequest bytes -> [(resource attributes, span dict)]."""
    out = []
    for fn, _wt, rs in _fields(body):
        if fn != 1:
            continue
        res_attrs: Dict[str, object] = {}
        scopes = []
        for f2, _w2, v2 in _fields(rs):
            if f2 == 1:  # Resource
                res_attrs = _attrs_pb([v for f3, _w3, v in _fields(v2) if f3 == 1])
            elif f2 == 2:  # ScopeSpans
                scopes.append(v2)
        for ss in scopes:
            for f3, _w3, sp in _fields(ss):
                if f3 != 2:
                    continue
                d: dict = {"attributes": []}
                attrs = []
                for f4, _w4, v4 in _fields(sp):
                    if f4 == 1:
                        d["traceId"] = bytes(v4)
                    elif f4 == 2:
                        d["spanId"] = bytes(v4)
                    elif f4 == 4:
                        d["parentSpanId"] = bytes(v4)
                    elif f4 == 5:
                        d["name"] = bytes(v4).decode("utf-8", "replace")
                    elif f4 == 6:
                        d["kind"] = v4
                    elif f4 == 7:
                        d["startTimeUnixNano"] = v4
                    elif f4 == 8:
                        d["endTimeUnixNano"] = v4
                    elif f4 == 9:
                        attrs.append(v4)
                    elif f4 == 15 and _w4 == 2:  # Status: 2 the message, 3 the code
                        for f5, w5, v5 in _fields(v4):
                            if f5 == 3 and w5 == 0:
                                d["statusCode"] = int(v5)
                d["attrs"] = _attrs_pb(attrs)
                out.append((res_attrs, d))
    return out


_STATUS_NAMES = {"STATUS_CODE_UNSET": 0, "STATUS_CODE_OK": 1, "STATUS_CODE_ERROR": 2}


def _status_code(v) -> int:
    """OTLP/JSON ``status.code``: an integer, or the enum's name; anything else is UNSET."""
    if isinstance(v, str):
        if v in _STATUS_NAMES:
            return _STATUS_NAMES[v]
        try:
            return int(v)
        except ValueError:
            return 0
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        return 0
    try:
        return int(v)
    except (ValueError, OverflowError):
        return 0


def _json_value(v: dict):
    if not isinstance(v, dict):
        return v
    for k in ("stringValue", "boolValue", "doubleValue"):
        if k in v:
            return v[k]
    if "intValue" in v:
        return int(v["intValue"])
    if "bytesValue" in v:
        return v["bytesValue"]
    return None


def _attrs_json(items) -> Dict[str, object]:
    return {a.get("key", ""): _json_value(a.get("value", {})) for a in (items or []) if a.get("key")}


def parse_json(body: bytes) -> List[Tuple[Dict[str, object], dict]]:
    """OTLP/JSON ExportTraceServiceRequest -> [(resource attributes, span dict)]."""
    doc = json.loads(body or b"{}")
    out = []
    for rs in doc.get("resourceSpans", []) or []:
        res_attrs = _attrs_json((rs.get("resource") or {}).get("attributes"))
        for ss in rs.get("scopeSpans", rs.get("instrumentationLibrarySpans", [])) or []:
            for sp in ss.get("spans", []) or []:
                d = dict(sp)
                d["attrs"] = _attrs_json(sp.get("attributes"))
                st = sp.get("status")
                if isinstance(st, dict) and st.get("code") is not None:
                    d["statusCode"] = _status_code(st.get("code"))
                out.append((res_attrs, d))
    return out


# ---------------------------------------------------------------------------------------
# span -> SPAN record mapping
# ---------------------------------------------------------------------------------------

@dataclass
class GroupTable:
    """service.name -> incident group id (first seen first); the last group collects overflow."""
    cap: int
    names: List[str] = field(default_factory=list)
    ids: Dict[str, int] = field(default_factory=dict)
    lock: threading.Lock = field(default_factory=threading.Lock)

    def id(self, service: str) -> int:
        with self.lock:
            g = self.ids.get(service)
            if g is None:
                if len(self.names) < self.cap:
                    g = len(self.names)
                    self.names.append(service)
                else:
                    g = self.cap - 1
                self.ids[service] = g
            return g


def _ipv4(v) -> int:
    """An IPv4 address as the probes hold it: the 4 network-order bytes the kernel stores
    (skc_daddr, the tcp tracepoint's daddr) read as a little-endian u32 -- REF's ipFromU32
    formats that value byte-wise (pkg/collector/ringbuf.go:240-243) -- so a span's connection
    hashes like the kernel records of the same connection."""
    try:
        a = ipaddress.ip_address(str(v))
    except ValueError:
        return 0
    return struct.unpack("<I", a.packed)[0] if a.version == 4 else 0


def _first(attrs: Dict[str, object], keys) -> object:
    for k in keys:
        if k in attrs and attrs[k] is not None:
            return attrs[k]
    return None


def _truthy(v: object) -> bool:
    return v is True or (isinstance(v, str) and v.lower() == "true") or (isinstance(v, (int, float)) and v == 1)


def tpot_us(attrs: Dict[str, object], ttft_ms: float, latency_ms: float) -> int:
    """A request span's time per output token in the record's integer microseconds (0: none), from
    the first that applies: ``llm.slo.tpot_ms``; ``llm.slo.tokens_per_sec`` = r > 0 as 1000 / r;
    ``gen_ai.usage.output_tokens`` = n >= 2 as (latency - TTFT) / (n - 1)."""
    try:
        v = attrs.get(semconv.ATTR_SLO_TPOT_MS)
        if v is not None:
            return records.tpot_us_of_ms(float(v))
        r = attrs.get(semconv.ATTR_SLO_TOKENS_PER_SEC)
        if r is not None:
            r = float(r)
            return records.tpot_us_of_ms(1000.0 / r) if r > 0.0 else 0
        n = attrs.get("gen_ai.usage.output_tokens")
        if n is not None and float(n) >= 2:
            return records.tpot_us_of_ms((float(latency_ms) - float(ttft_ms)) / (float(n) - 1.0))
    except (TypeError, ValueError):
        pass
    return 0


def _number(v) -> Optional[int]:
    """A status code attribute as an integer; ``None`` for what is no whole number."""
    if isinstance(v, bool) or not isinstance(v, (int, float, str)):
        return None
    try:
        x = float(v)
    except (TypeError, ValueError):
        return None
    if not np.isfinite(x) or x != int(x):
        return None
    return int(x)


_HTTP_CLASS = {429: records.OUTCOME_THROTTLED, 408: records.OUTCOME_TIMEOUT, 504: records.OUTCOME_TIMEOUT,
               499: records.OUTCOME_CANCELLED, 502: records.OUTCOME_UNAVAILABLE, 503: records.OUTCOME_UNAVAILABLE}
_GRPC_CLASS = {1: records.OUTCOME_CANCELLED, 4: records.OUTCOME_TIMEOUT, 8: records.OUTCOME_THROTTLED,
               14: records.OUTCOME_UNAVAILABLE,
               **{c: records.OUTCOME_SERVER for c in (2, 10, 12, 13, 15)},
               **{c: records.OUTCOME_CLIENT for c in (3, 5, 6, 7, 9, 11, 16)}}


def outcome_class(attrs: Dict[str, object], status_code: object = None) -> int:
    """A finished request's outcome class (records.OUTCOME_*, 0 = ok). The first source that yields a
    non-zero class decides: the HTTP status (``http.response.status_code``, else ``http.status_code``);
    ``rpc.grpc.status_code``; ``error.type``; the span status ERROR or a truthy ``llm.slo.error``. A value
    that is not a number where one is expected yields nothing."""
    h = attrs.get("http.response.status_code")
    if h is None:
        h = attrs.get("http.status_code")
    h = _number(h)
    if h is not None and h >= 400:
        c = _HTTP_CLASS.get(h)
        if c is None:
            c = records.OUTCOME_SERVER if 500 <= h <= 599 else (records.OUTCOME_CLIENT if h <= 499 else 0)
        if c:
            return c
    c = _GRPC_CLASS.get(_number(attrs.get("rpc.grpc.status_code")), 0)
    if c:
        return c
    e = attrs.get("error.type")
    if isinstance(e, str) and e:
        e = e.lower()
        if "cancel" in e:
            return records.OUTCOME_CANCELLED
        if "timeout" in e or "deadline" in e:
            return records.OUTCOME_TIMEOUT
        if "throttl" in e or "rate_limit" in e or "ratelimit" in e:
            return records.OUTCOME_THROTTLED
        return records.OUTCOME_OTHER
    if _number(status_code) == 2 or _truthy(attrs.get(semconv.ATTR_SLO_ERROR)):
        return records.OUTCOME_OTHER
    return records.OUTCOME_OK


class SpanMapper:
    """OTLP spans -> SPAN records on the agent's ids."""

    def __init__(self, groups: GroupTable, pod_id: Callable[[str], int], node_id: int = 0,
                 pod_ips: Optional[Callable[[], Dict[str, set]]] = None, forwarders: str = "",
                 decode_sli: bool = False, error_sli: bool = False):
        """``pod_ips()`` -> {IP: pod uids at that IP} of this node's pods (procfs.pod_addresses):
        a span that names a pod is kept only when it comes from that pod's address (or from an
        address the map does not know). ``forwarders``: CIDRs of trusted span forwarders (an
        OpenTelemetry collector relaying many pods' spans) the address check does not apply to.
        ``decode_sli``: a request span's time per output token goes into bits 8-31 of its ``flags``
        (``tpot_us``); off, the records are what they were. ``error_sli``: the record that ends a request
        gets the request's outcome class in bits 4-7 of its ``flags`` (``outcome_class``), with or without
        a TTFT; off, the records are what they were."""
        self.groups, self.pod_id, self.node_id = groups, pod_id, node_id
        self.decode_sli = bool(decode_sli)
        self.error_sli = bool(error_sli)
        self.pod_ips = pod_ips
        self.forwarders = [ipaddress.ip_network(c.strip(), strict=False) for c in forwarders.split(",") if c.strip()]
        self.conflicts = 0  # spans that named a pod already bound to another service (dropped)
        self.spoofed = 0    # spans from a known pod address naming another pod (dropped)
        # pod id -> svc << 16 | node as the spans reveal it: the window engine's pod table, so the
        # kernel's and the rocprof tool's records of a pod carry its service (the service+node join
        # tier, and the service that decides which GPU owns them, agent --gpus N)
        self._pods: Dict[int, int] = {}
        self._new: Dict[int, int] = {}
        self._plock = threading.Lock()
        # late breaches (records.SPAN_LATE): the agent sets slo_ms, and late_before_ns at every window
        # cut; a span whose TTFT-SLO deadline (start + slo) lies before it is flagged -- if it
        # breached, the breach belongs to an earlier window than the one it is reported in
        self.slo_ms = 0.0
        self.late_before_ns = 0
        # retrieval breakdowns of traces whose request span has not arrived yet (bounded, oldest out)
        self._retr: "collections.OrderedDict[int, float]" = collections.OrderedDict()
        self._rlock = threading.Lock()
        self.retrieval_cap = 8192
        # first-token records (llm.slo.ttft_early): a request's SLI as soon as its first token is
        # out, not when the request span ends -- the breach reaches the window it happened in. The
        # traces counted that way (and, for the rare early record that comes second, the traces
        # whose request span counted already), bounded, oldest out
        self._early: "collections.OrderedDict[int, bool]" = collections.OrderedDict()
        self._final: "collections.OrderedDict[int, bool]" = collections.OrderedDict()
        self.early_dropped = 0  # first-token records after their request span (counted by it)
        # request exemplars (agent --request-exemplars): ``trace_h`` is the low 64 bits of the W3C id;
        # with this set the high half of every record's id is remembered, bounded, oldest out. Off:
        # nothing is kept
        self.keep_trace_high = False
        self._high: "collections.OrderedDict[int, int]" = collections.OrderedDict()

    def trace_high(self, trace_h: int) -> Optional[int]:
        """The high 64 bits of the W3C trace id whose low half is ``trace_h``, while remembered."""
        with self._rlock:
            return self._high.get(int(trace_h))

    def take_pod_updates(self) -> Optional[Tuple[np.ndarray, np.ndarray]]:
        """(pod ids, svc|node) learned since the last call, or None."""
        with self._plock:
            if not self._new:
                return None
            new, self._new = self._new, {}
        ids = np.array(list(new), dtype=np.uint32)
        return ids, np.array([new[int(i)] for i in ids.tolist()], dtype=np.uint32)

    def _forwarder(self, peer: str) -> bool:
        try:
            ip = ipaddress.ip_address(peer)
        except ValueError:
            return False
        return any(ip in n for n in self.forwarders)

    @staticmethod
    def is_request_span(d: dict) -> bool:
        attrs = d.get("attrs", {})
        return (not d.get("parentSpanId") or any(k in attrs for k in TTFT_KEYS)
                or _truthy(attrs.get(semconv.ATTR_SLO_REQUEST_START)))

    def records(self, spans: List[Tuple[Dict[str, object], dict]], peer: str = "") -> np.ndarray:
        """Request spans -> SPAN records. A pod's service is bound by the first span that names
        both; later spans naming that pod with another service are dropped (a pod cannot move
        another pod's records to its service), and with ``pod_ips`` a span naming a pod must come
        from that pod's address when the address is one of this node's pods."""
        sel = [(r, d) for r, d in spans if self.is_request_span(d)]
        # the retrieval breakdowns of this export's spans, summed per trace
        retr: Dict[int, float] = {}
        for _r, d in spans:
            v = retrieval_ms(d.get("attrs", {}))
            if v is not None:
                th = trace_hash(d.get("traceId"))
                if th:
                    retr[th] = retr.get(th, 0.0) + v
        if retr:
            req = {trace_hash(d.get("traceId")) for _r, d in sel}
            with self._rlock:
                for th, v in retr.items():
                    if th not in req:  # its request span comes later: wait for it
                        self._retr[th] = self._retr.pop(th, 0.0) + v
                while len(self._retr) > self.retrieval_cap:
                    self._retr.popitem(last=False)
        at_peer = None
        if self.pod_ips is not None and peer and not self._forwarder(peer):
            try:
                at_peer = self.pod_ips().get(peer)
            except Exception:  # noqa: BLE001 - an unreadable map checks nothing
                at_peer = None
        # per-field lists, written into the record array column by column at the end: setting the
        # fields of one structured element at a time cost ~18 us per span (the receiver's CPU)
        ts, tr, sh, pids, pods, svcs, grps, ttft, lat, conn, rms, flags = ([] for _ in range(12))
        late_before, slo_ns = int(self.late_before_ns), int(round(float(self.slo_ms) * 1e6))
        res_cache: Dict[int, tuple] = {}  # one resource's service / pod / pid per request
        groups_seen: Dict[str, int] = {}
        pods_seen: Dict[object, int] = {}
        for res, d in sel:
            a = d["attrs"]
            t0 = int(d.get("startTimeUnixNano") or 0)
            t1 = int(d.get("endTimeUnixNano") or t0)
            rk = id(res)
            rv = res_cache.get(rk)
            if rv is None:
                rv = res_cache[rk] = (_first(res, ("service.name",)), _first(res, ("k8s.pod.uid",)) or
                                      _first(res, ("k8s.pod.name",)) or "", _first(res, ("process.pid",)))
            svc = str(rv[0] or _first(a, ("service.name",)) or "unknown")
            pod = rv[1]
            gk = groups_seen.get(svc)
            pid = rv[2] or _first(a, ("process.pid", "thread.id")) or 0
            if pod and at_peer is not None and str(pod) not in at_peer:
                self.spoofed += 1
                continue
            if gk is None:
                gk = groups_seen[svc] = self.groups.id(svc)
            g = gk
            pid_ = pods_seen.get(pod)
            if pid_ is None:
                pid_ = pods_seen[pod] = self.pod_id(str(pod)) if pod else 0
            if pid_:
                sn = ((g + 1) << 16) | (self.node_id & 0xFFFF)
                bound = self._pods.get(pid_)
                if bound is not None and bound != sn:
                    self.conflicts += 1
                    continue
                if bound is None:
                    with self._plock:
                        self._pods[pid_] = sn
                        self._new[pid_] = sn
            sport = _first(a, ("client.port", "net.host.port", "net.sock.host.port")) or 0
            dport = _first(a, ("server.port", "net.peer.port", "net.sock.peer.port")) or 0
            v = _first(a, TTFT_KEYS)
            th = trace_hash(d.get("traceId"))
            if self.keep_trace_high and th:
                hi = trace_high_half(d.get("traceId"))
                if hi is not None:
                    with self._rlock:
                        self._high[th] = hi
                        self._high.move_to_end(th)
                        while len(self._high) > self.retrieval_cap:
                            self._high.popitem(last=False)
            fl = 0
            # a start record (llm.slo.request_start, no TTFT yet): joins, never counts, and leaves
            # the first-token / request-span pairing and the trace's retrieval breakdown alone
            start = v is None and _truthy(a.get(semconv.ATTR_SLO_REQUEST_START))
            if start:
                fl = records.SPAN_START | records.SPAN_NO_SLI
            elif th and v is not None:
                if _truthy(a.get(semconv.ATTR_SLO_TTFT_EARLY)):
                    with self._rlock:
                        if self._final.pop(th, None) is not None:
                            self.early_dropped += 1
                            continue
                        self._early[th] = True
                        while len(self._early) > self.retrieval_cap:
                            self._early.popitem(last=False)
                    fl = records.SPAN_FIRST_TOKEN
                else:
                    with self._rlock:
                        if self._early.pop(th, None) is not None:
                            fl = records.SPAN_NO_SLI
                        else:
                            self._final[th] = True
                            while len(self._final) > self.retrieval_cap:
                                self._final.popitem(last=False)
            # the decode SLI rides on the request span: the record that ends the request, not its start
            # or first-token record (one without a trace id carries no flag, but is no request span either)
            if self.decode_sli and not start and v is not None and not _truthy(a.get(semconv.ATTR_SLO_TTFT_EARLY)):
                fl |= records.pack_tpot_us(tpot_us(a, float(v), (t1 - t0) / 1e6))
            # the outcome rides on the record that ends the request too, but needs no TTFT: a failed
            # request usually has none
            if self.error_sli and not (fl & (records.SPAN_START | records.SPAN_FIRST_TOKEN)):
                fl |= records.pack_outcome(outcome_class(a, d.get("statusCode")))
            flags.append(fl)
            # the trace's retrieval breakdown goes to its first record (a first-token record when the
            # service exports one), once: later records of the trace carry only what arrives with them
            rv = retr.pop(th, None) if th and not start else None
            if self._retr and th and not start:
                with self._rlock:
                    early = self._retr.pop(th, None)
                if early is not None:
                    rv = (rv or 0.0) + early
            rms.append(rv if rv is not None else 0.0)
            ts.append(t0)
            tr.append(th)
            sh.append(span_hash(d.get("spanId")))
            pids.append(int(pid))
            pods.append(pid_)
            svcs.append(g + 1)
            grps.append(g)
            ttft.append(float(v) if v is not None else np.nan)
            lat.append((t1 - t0) / 1e6)
            if int(sport) or int(dport):
                dip = _ipv4(_first(a, ("server.address", "net.peer.ip", "net.sock.peer.addr")) or "")
                conn.append(records.conn_hash(int(sport), int(dport), dip))
            else:
                conn.append(0)
        out = np.zeros(len(ts), dtype=records.SPAN)
        if ts:
            out["ts_ns"] = ts
            out["trace_h"] = np.array(tr, dtype=np.uint64)
            out["span_h"] = np.array(sh, dtype=np.uint64)
            out["pid"] = pids
            out["pod_id"] = pods
            out["node_id"] = self.node_id
            out["svc_id"] = svcs
            out["group_id"] = grps
            out["ttft_ms"] = ttft
            out["latency_ms"] = lat
            out["conn_h"] = np.array(conn, dtype=np.uint64)
            out["retr_ms"] = rms
            fl = np.asarray(flags, dtype=np.uint32)
            if late_before > 0 and slo_ns > 0:
                t0s = np.asarray(ts, dtype=np.int64)
                fl |= np.where((t0s > 0) & (t0s + slo_ns < late_before) & ((fl & records.SPAN_START) == 0),
                               records.SPAN_LATE, 0).astype(np.uint32)
            out["flags"] = fl
        return out


class _Headers(dict):
    """Request headers by lower-cased name, with the case-insensitive ``get`` of http.client's."""

    def get(self, key, default=None):
        return super().get(key.lower(), default)


class OtlpSpanReceiver:
    """POST /v1/traces -> span ring. ``push(records) -> n accepted`` is the ring's push (the
    span ring is multi-producer: services may also push records directly)."""

    MAX_BODY = 4 << 20  # bytes per export request (OTLP exporters batch well below this)

    def __init__(self, bind: str, mapper: SpanMapper, push: Callable[[np.ndarray], int], allow: str = "",
                 max_body: int = MAX_BODY):
        """``allow``: comma-separated CIDRs of peers that may export (empty = any): the agent binds
        on the host network, so without it any node that reaches the port could inject spans."""
        self.mapper, self.push = mapper, push
        host, _, port = bind.rpartition(":")
        self.addr = (host or "127.0.0.1", int(port))
        self.max_body = int(max_body)
        self.allow = [ipaddress.ip_network(c.strip(), strict=False) for c in allow.split(",") if c.strip()]
        self.accepted = self.rejected = self.dropped = self.requests = 0
        self.refused = 0  # peers outside the allow-list, oversized or unframed bodies
        self._peer_ok: Dict[str, bool] = {}
        self._lock = threading.Lock()
        self._srv: Optional[http.server.ThreadingHTTPServer] = None
        self._thr: Optional[threading.Thread] = None

    def ingest(self, body: bytes, content_type: str, peer: str = "") -> Tuple[int, int]:
        """Parse one export request and push its request spans; (pushed, dropped)."""
        ct = (content_type or "").split(";")[0].strip().lower()
        spans = parse_proto(body) if ct in ("application/x-protobuf", "application/protobuf") else parse_json(body)
        recs = self.mapper.records(spans, peer)
        n = int(self.push(recs)) if len(recs) else 0
        with self._lock:
            self.requests += 1
            self.accepted += n
            self.dropped += len(recs) - n
        return n, len(recs) - n

    def start(self) -> "OtlpSpanReceiver":
        rx = self

        class H(http.server.BaseHTTPRequestHandler):
            protocol_version = "HTTP/1.1"

            def log_message(self, *a):  # noqa: D401 - quiet
                pass

            def parse_request(self) -> bool:
                """The request line and headers without the email-package parser
                (http.client.parse_headers: ~0.3 ms of the receiver's ~1.4 ms per export request):
                exporters send a handful of plain headers; anything unusual falls back to it."""
                line = str(self.raw_requestline, "iso-8859-1").rstrip("\r\n")
                parts = line.split()
                if len(parts) != 3 or not parts[2].startswith("HTTP/1."):
                    return super().parse_request()
                self.command, self.path, self.request_version = parts
                self.requestline = line
                hdrs = _Headers()
                for _ in range(100):
                    raw = self.rfile.readline(65537)
                    if len(raw) > 65536:
                        self.send_error(431, "Line too long")
                        return False
                    if raw in (b"\r\n", b"\n", b""):
                        break
                    k, sep, v = raw.decode("iso-8859-1").partition(":")
                    if not sep:
                        self.send_error(400, "Bad header line")
                        return False
                    name = k.strip().lower()
                    if name in hdrs and name in ("content-length", "transfer-encoding", "host"):
                        self.close_connection = True  # conflicting framing: never guess which one
                        self.send_error(400, "Duplicate header")
                        return False
                    hdrs[name] = v.strip()
                else:
                    self.send_error(431, "Too many headers")
                    return False
                self.headers = hdrs
                conn = hdrs.get("connection", "").lower()
                self.close_connection = conn == "close" or (self.request_version == "HTTP/1.0" and conn != "keep-alive")
                if hdrs.get("expect", "").lower() == "100-continue":
                    self.send_response_only(100)
                    self.end_headers()
                return True

            def _reply(self, code: int, body: bytes, ctype: str) -> None:
                # one write: status line, headers and body (send_response formats a Date header
                # and buffers per header)
                head = (f"HTTP/1.1 {code} {self.responses.get(code, ('',))[0]}\r\nContent-Type: {ctype}\r\n"
                        f"Content-Length: {len(body)}\r\n" + ("Connection: close\r\n" if self.close_connection else "")
                        + "\r\n")
                self.wfile.write(head.encode("latin-1") + body)

            def _refuse(self, code: int, msg: bytes) -> None:
                with rx._lock:
                    rx.refused += 1
                self.close_connection = True
                self._reply(code, msg, "text/plain")

            def do_POST(self):
                if rx.allow:
                    host = self.client_address[0]
                    ok = rx._peer_ok.get(host)
                    if ok is None:  # decided once per peer address (ipaddress parsing is slow)
                        try:
                            peer = ipaddress.ip_address(host)
                        except ValueError:
                            peer = None
                        ok = peer is not None and any(peer in net for net in rx.allow)
                        if len(rx._peer_ok) < 4096:
                            rx._peer_ok[host] = ok
                    if not ok:
                        self._refuse(403, b"forbidden")
                        return
                if not self.path.startswith("/v1/traces"):
                    self._reply(404, b"not found", "text/plain")
                    return
                if self.headers.get("Transfer-Encoding") is not None:  # chunked bodies are not accepted
                    self._refuse(411, b"length required")
                    return
                try:
                    n = int(self.headers.get("Content-Length", ""))
                except ValueError:  # chunked or missing: the body size must be known up front
                    self._refuse(411, b"length required")
                    return
                if n < 0 or n > rx.max_body:  # refused before a byte of it is read
                    self._refuse(413, b"request body too large")
                    return
                body = self.rfile.read(n) if n > 0 else b""
                ctype = self.headers.get("Content-Type", "application/json")
                try:
                    _, dropped = rx.ingest(body, ctype, str(self.client_address[0]))
                except (ValueError, KeyError, TypeError) as exc:
                    with rx._lock:
                        rx.rejected += 1
                    self._reply(400, json.dumps({"error": str(exc)}).encode(), "application/json")
                    return
                if ctype.startswith("application/x-protobuf"):
                    # ExportTraceServiceResponse{partial_success{rejected_spans}}: empty when none
                    inner = b"\x08" + _enc_varint(dropped)
                    msg = b"" if not dropped else b"\x0a" + _enc_varint(len(inner)) + inner
                    self._reply(200, msg, "application/x-protobuf")
                else:
                    body = {} if not dropped else {"partialSuccess": {"rejectedSpans": str(dropped),
                                                                      "errorMessage": "span ring full"}}
                    self._reply(200, json.dumps(body).encode(), "application/json")

        self._srv = http.server.ThreadingHTTPServer(self.addr, H)
        self._srv.daemon_threads = True
        self.addr = self._srv.server_address[:2]
        self._thr = threading.Thread(target=self._srv.serve_forever, name="otlp-receiver", daemon=True)
        self._thr.start()
        return self

    @property
    def endpoint(self) -> str:
        return f"http://{self.addr[0]}:{self.addr[1]}/v1/traces"

    def stop(self) -> None:
        if self._srv is not None:
            self._srv.shutdown()
            self._srv.server_close()
            self._srv = None


def _enc_varint(v: int) -> bytes:
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)
