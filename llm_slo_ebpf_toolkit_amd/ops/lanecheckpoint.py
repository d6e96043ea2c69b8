"""Checkpoint calls every device side tracker's handle shares: the step lane under the native class
(ops/csrc/steplane.h) saves and restores the tracker's arrays without knowing the tracker, so the eleven
handles forward the same four calls. docs/TRACKER_CHECKPOINT.md has the format and the rules."""

from __future__ import annotations

import numpy as np

FORMAT = "mislo-lane-image/1"


class LaneCheckpoint:
    """``self.t`` is the native tracker. The image is the device's own format (header, then the arrays);
    pipeline/trackerstate.py's oracle format is another."""

    def snapshot(self) -> int:
        """Enqueue a snapshot behind the steps issued so far: a kernel gathers and digests the state on the
        tracker's stream, the transfer to the host runs beside the steps that follow. Returns a ticket; a
        second snapshot while one is unread is refused (RuntimeError)."""
        return int(self.t.snapshot())

    def snapshot_ready(self, ticket: int) -> bool:
        return bool(self.t.snapshot_ready(int(ticket)))

    def snapshot_image(self, ticket: int) -> np.ndarray:
        """The image of snapshot ``ticket`` as uint8 (waits for the transfer)."""
        return np.frombuffer(self.t.snapshot_image(int(ticket)), dtype=np.uint8)

    def restore(self, image) -> int:
        """Resume from an image, before the first step only. ``ValueError`` names what does not fit (another
        tracker, another configuration field, a truncated or damaged image) and nothing has changed. Returns
        the index the next step gets; the steps before it are not held."""
        return int(self.t.restore(np.ascontiguousarray(np.frombuffer(bytes(image), dtype=np.uint8)
                                                       if isinstance(image, (bytes, bytearray, memoryview))
                                                       else np.asarray(image, dtype=np.uint8).reshape(-1))))

    # ---- the same pair the numpy oracles have (pipeline/trackerstate.py), for WindowPipeline ----
    def state(self):
        """``({"image": uint8}, meta)``: a snapshot taken now and waited for; ``meta`` holds the header's kind,
        fingerprint and step index and the image's bytes."""
        image = self.snapshot_image(self.snapshot())
        return {"image": image}, self.image_meta(image)

    @staticmethod
    def image_meta(image) -> dict:
        from . import load_agent

        kind, fingerprint, step, _segs, _fields, _host, _payload, _digest = load_agent().lane_image_header(image)
        return {"format": FORMAT, "kind": str(kind), "fingerprint": f"{int(fingerprint):016x}", "step": int(step),
                "bytes": int(len(image))}

    def restore_state(self, arrays, meta) -> int:
        """``restore`` of ``state()``'s pair; an oracle's state is refused by its format."""
        if meta.get("format") != FORMAT:
            raise ValueError(f"tracker image: format {meta.get('format')!r}, the device tracker reads {FORMAT!r}")
        return self.restore(arrays["image"])

    def image_bytes(self) -> int:
        return int(self.t.image_bytes())

    def snapshot_kernel_ms(self) -> float:
        """Device time of the last read snapshot's gather and digest kernel, ms."""
        return float(self.t.snapshot_kernel_ms())
