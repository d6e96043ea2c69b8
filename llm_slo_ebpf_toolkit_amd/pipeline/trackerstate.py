"""Checkpoint and resume of a side tracker's numpy oracle: ``state() -> (arrays, meta)`` and
``restore(arrays, meta)`` for all eleven oracles from one helper (docs/TRACKER_CHECKPOINT.md).

An oracle names what it keeps: ``KIND`` (the tracker's name as its messages spell it), ``FINGERPRINT``
(the attributes that shape the state or its meaning -- the fields ops/csrc/*_host.h fingerprint() covers,
under the constructor's names; not device, n_buffers, span_cap or lds) and ``STATE`` (the attributes kept
between steps, the step counter ``n`` among them). The helper walks those attributes: numpy arrays
(structured ones too) go into one ``image`` of bytes, integers, floats, ``None``, lists, tuples, deques and dicts with integer keys into
``meta["spec"]``. The format is the oracle's own: the device tracker's image (ops/csrc/steplane_host.h) is
another, and ``meta["kind"]`` refuses the mix. Loading executes nothing from the image.
"""

from __future__ import annotations

from collections import deque
from typing import Dict, List, Tuple

import numpy as np

FORMAT = "mislo-oracle-state/1"


def _plain(v):
    """A fingerprint value as JSON carries it."""
    if isinstance(v, np.generic):
        return v.item()
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in sorted(v.items())}
    return v


def _descr(dt: np.dtype):
    return dt.str if dt.names is None else [list(x) if not isinstance(x, str) else x for x in _plain(dt.descr)]


def _dtype(d) -> np.dtype:
    return np.dtype(d) if isinstance(d, str) else np.dtype([tuple(tuple(y) if isinstance(y, list) else y for y in x)
                                                            for x in d])


def _encode(v, chunks: List[bytes], at: List[int]):
    if isinstance(v, np.ndarray):
        b = np.ascontiguousarray(v).tobytes()
        spec = {"a": [at[0], len(b)], "dtype": _descr(v.dtype), "shape": list(v.shape)}
        chunks.append(b)
        at[0] += len(b)
        return spec
    if isinstance(v, (bool, np.bool_)):
        return {"b": bool(v)}
    if isinstance(v, (int, np.integer)):
        return {"i": int(v)}
    if isinstance(v, (float, np.floating)):
        return {"f": float(v).hex()}
    if v is None:
        return {"none": 1}
    if isinstance(v, (list, tuple, deque)):
        kind = "deque" if isinstance(v, deque) else "tuple" if isinstance(v, tuple) else "list"
        return {kind: [_encode(x, chunks, at) for x in v]}
    if isinstance(v, dict):
        return {"dict": [[int(k), _encode(x, chunks, at)] for k, x in v.items()]}
    raise TypeError(f"tracker state: cannot save a {type(v).__name__}")


def _decode(spec, image: np.ndarray):
    if "a" in spec:
        off, n = (int(x) for x in spec["a"])
        dt, shape = _dtype(spec["dtype"]), tuple(int(x) for x in spec["shape"])
        if off < 0 or n < 0 or off + n > len(image) or n != dt.itemsize * int(np.prod(shape, dtype=np.int64)):
            raise ValueError("tracker state: an array lies outside the image")
        return np.frombuffer(image[off:off + n].tobytes(), dtype=dt).reshape(shape).copy()
    if "b" in spec:
        return bool(spec["b"])
    if "i" in spec:
        return int(spec["i"])
    if "f" in spec:
        return float.fromhex(spec["f"])
    if "none" in spec:
        return None
    for kind, make in (("list", list), ("tuple", tuple), ("deque", deque)):
        if kind in spec:
            return make(_decode(x, image) for x in spec[kind])
    if "dict" in spec:
        return {int(k): _decode(x, image) for k, x in spec["dict"]}
    raise ValueError("tracker state: an entry of no known type")


class OracleCheckpoint:
    """``state`` / ``restore`` of an oracle from its ``KIND``, ``FINGERPRINT`` and ``STATE`` tuples."""

    KIND = ""
    FINGERPRINT: Tuple[str, ...] = ()
    STATE: Tuple[str, ...] = ()

    def fingerprint(self) -> Dict[str, object]:
        """Field name -> value. An entry of FINGERPRINT is an attribute's name, ``(field, attribute)`` where the
        two differ, or the name of a dict of fields (its entries count one by one)."""
        out: Dict[str, object] = {}
        for entry in self.FINGERPRINT:
            name, attr = (entry, entry) if isinstance(entry, str) else entry
            v = getattr(self, attr)
            if isinstance(v, dict):
                out.update({str(k): _plain(x) for k, x in v.items()})
            else:
                out[name] = _plain(v)
        return out

    def state(self) -> Tuple[Dict[str, np.ndarray], Dict[str, object]]:
        """Everything kept between steps: ``({"image": uint8}, meta)``. The held results are not state."""
        chunks: List[bytes] = []
        at = [0]
        spec = {name: _encode(getattr(self, name), chunks, at) for name in self.STATE}
        image = np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()
        meta = {"format": FORMAT, "kind": self.KIND, "fingerprint": self.fingerprint(), "step": int(self.n),
                "bytes": int(len(image)), "spec": spec}
        return {"image": image}, meta

    def check_state(self, meta: Dict[str, object]) -> None:
        """``ValueError`` naming what differs when ``meta`` is not a state this oracle can take."""
        who = f"{self.KIND} image: "
        if meta.get("format") != FORMAT:
            raise ValueError(f"{who}format {meta.get('format')!r}, this oracle reads {FORMAT!r}")
        if meta.get("kind") != self.KIND:
            raise ValueError(f"{who}kind {meta.get('kind')}, this tracker {self.KIND}")
        saved, mine = meta.get("fingerprint") or {}, self.fingerprint()
        for name in mine:
            if name not in saved or saved[name] != mine[name]:
                raise ValueError(f"{who}{name} {saved.get(name)}, this tracker {mine[name]}")
        if set(meta.get("spec") or {}) != set(self.STATE):
            raise ValueError(f"{who}the saved attributes are not this oracle's")

    def restore(self, arrays: Dict[str, np.ndarray], meta: Dict[str, object]) -> int:
        """Resume from ``state()``, before the first step only; a refusal has changed nothing. Returns the
        index the next step gets; the steps before it are not held."""
        if self.n != 0 or self.res:
            raise RuntimeError(f"{self.KIND}: restore is only possible before the first step")
        self.check_state(meta)
        image = np.ascontiguousarray(arrays["image"], dtype=np.uint8).reshape(-1)
        if len(image) != int(meta.get("bytes", -1)):
            raise ValueError(f"{self.KIND} image: {len(image)} bytes, the state holds {meta.get('bytes')}")
        values = {name: _decode(meta["spec"][name], image) for name in self.STATE}  # all of it, or nothing
        for name, v in values.items():
            mine = getattr(self, name)
            if isinstance(mine, np.ndarray) and (not isinstance(v, np.ndarray) or v.dtype != mine.dtype
                                                 or v.shape != mine.shape):
                raise ValueError(f"{self.KIND} image: {name} has another shape or type")
        for name, v in values.items():
            setattr(self, name, v)
        self.res = {}
        return int(self.n)

    restore_state = restore
