"""Host-side mirror of Shock's request.Streamer, backed by libshockidx.

Reference (paths relative to shock-server/):
    request/streamer.go:39-49    type Streamer struct { R []file.SectionReader; ...; Filter filter.FilterFunc;
                                 ...; E error; ESection int }
    request/streamer.go:78-98    Stream: every SectionReader of R piped into one stream, in order, each
                                 through a new filter reader when Filter is set (s.Filter(sr), :86-90);
                                 the first io.Copy error is kept in E, its section in ESection, and the
                                 pipe ends there (:91-96)
    callers: controller/node/single.go:397-400, 442-444, 457-460 (part downloads) and :505-516 (a
             subset node: R is every row Idx.Range returns)

Same names: Streamer(R=[(pos, len), ...], Filter=name_or_None).Stream(node_bytes) returns a reader that
yields the bytes the client would receive and then raises ShockIndexError (Go's text) when a section's
reader failed; E and ESection are set as the goroutine sets them.  Filter takes the filter's name
("fq2fa", "anonymize"; filter.go:13-16) where the reference takes the FilterFunc it looked up by that
name.  The whole list goes to the device in one call (shockidx_stream_filter_device).
"""
from __future__ import annotations

import numpy as np

from . import _lib as L
from .filter import FilterReader, Has, _section_bytes
from .indexer import ShockIndexError, context


class DeviceSections:
    """count records {int64 pos, int64 len} in a DeviceBuffer (None when count is 0)."""

    def __init__(self, buf, count: int):
        self.buf = buf
        self.count = int(count)

    def __len__(self) -> int:
        return self.count

    def tolist(self):
        """the sections on the host (a copy: for inspection, the stream does not need it)"""
        if not self.count:
            return []
        return [tuple(r) for r in self.buf.rows(self.count).view(np.int64).tolist()]


class Streamer:
    def __init__(self, R, Filter: str | None = None, Size: int | None = None):  # noqa: N803  (streamer.go:39-49)
        if Filter is not None and not Has(Filter):
            raise KeyError(Filter)
        self.R = R if isinstance(R, DeviceSections) else [(int(p), int(n)) for p, n in R]
        self.Filter = Filter
        self.Size = Size  # streamer.go:46: the caller's sum of the section lengths (single.go:484)
        self.E: ShockIndexError | None = None
        self.ESection = 0  # Go's zero value; meaningful when E is set (streamer.go:92-95)

    def _stream_device(self, node):
        """the node to HBM, the device-resident sections through shockidx_stream_filter_device"""
        ctx = context()
        data = _section_bytes(node)
        d_in = ctx.alloc(len(data) + 64)
        d_in.upload(data)
        cap = 2 * max(int(self.Size or 0), 0) + 64  # anonymize may lengthen short records
        d_out = ctx.alloc(cap)
        d_secs = self.R.buf.ptr if self.R.count else None
        try:
            r = ctx.stream_filter_device(self.Filter, d_in.ptr, len(data), d_secs, self.R.count, d_out.ptr, cap)
            if r.status == L.ESPACE:  # r.size holds the bytes needed
                d_out.free()
                cap = int(r.size) + 64
                d_out = ctx.alloc(cap)
                r = ctx.stream_filter_device(self.Filter, d_in.ptr, len(data), d_secs, self.R.count, d_out.ptr, cap)
            if r.status in (L.OK, L.EFORMAT):
                r.gathered = d_out.download(r.size).tobytes() if r.size else b""
        finally:
            d_in.free()
            d_out.free()
        return r

    def Stream(self, node) -> FilterReader:  # noqa: N802  (streamer.go:78-98)
        if isinstance(self.R, DeviceSections):
            r = self._stream_device(node)
        else:
            r = context().stream_filter_host(self.Filter, _section_bytes(node), self.R)
        if r.status not in (L.OK, L.EFORMAT):
            raise RuntimeError(f"shockidx_stream_filter_device: {r.status} {r.err!r}")
        self.E, self.ESection = None, 0
        if r.status == L.EFORMAT:
            self.E = ShockIndexError(r.err)
            self.ESection = r.err_section
        return FilterReader(r.gathered or b"", r.err if r.status == L.EFORMAT else None)
