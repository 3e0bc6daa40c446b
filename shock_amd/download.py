"""Host-side mirror of the index branch of a node download, backed by libshockidx.

Reference (paths relative to shock-server/):
    controller/node/single.go:343-484   ?download&index=X[&part=a&part=b...]: the index is looked up
                                        (n.DynamicIndex), a virtual index gets its chunk_size
                                        (:350-367), then the Streamer's section list s.R is built part
                                        by part (:372-483) and s.Size is the sum of the lengths (:484)
    node/file/index/virtual.go:50-80    SizePart, the virtual "size" index

Download(...) takes what the controller reads from the node and the query -- the node type, the index
name, IdxInfo.Type and TotalUnits, the .idx path(s), the `part` values, chunk_size, the file size --
picks the branch the controller takes and returns (Streamer, err): every part goes through one
shockidx_download_plan call, the sections stay on the device (Streamer.R is a DeviceSections) and
Streamer.Size is Go's `size`.  err is a ShockIndexError with the text the controller responds with:
Go's index errors (IndexNoFile, InvalidIndexRange, IndexOutBounds; err.part is the failing part), the
empty-node IndexOutBounds (:463-466), "record index must exist" (:377), the virtual-index refusal for
subset nodes (:352) and "requires part parameter" (:428, :479).  The .idx tables are served from the
HBM cache of shock_amd.index.
"""
from __future__ import annotations

from . import _lib as L
from .core import _go_i64
from .index import _tables
from .indexer import ShockIndexError, context
from .stream import DeviceSections, Streamer

CHUNK_SIZE = 1048576  # conf.CHUNK_SIZE (single.go:357)
E_INDEX_OUT_BOUNDS = b"Index record out of bounds"
E_RECORD_INDEX = b"Invalid request, record index must exist to retrieve chunkrecord index on a subset node."
E_VIRTUAL_SUBSET = b"subset nodes do not currently support virtual indices"
E_NEEDS_PART = b"Index parameter requires part parameter"


def _err(msg: bytes, part: int = -1):
    e = ShockIndexError(msg)
    e.part = part
    return None, e


def _plan(mode, parts, idx_path=None, total_units=0, rec_path=None, rec_total_units=0, file_size=0, chunk_size=0,
          Filter=None):  # noqa: N803
    ctx = context()
    t = _tables.get(idx_path) if idx_path is not None else None
    d_rows, nrows = t if t is not None else (None, 0)
    t = _tables.get(rec_path) if rec_path is not None else None
    d_rec, rec_nrows = t if t is not None else (None, 0)
    args = (mode, list(parts), d_rows, nrows, total_units, d_rec, rec_nrows, rec_total_units, file_size, chunk_size)
    r = ctx.download_plan(*args)  # sizes the list: ESPACE carries the sections needed
    buf = None
    if r.status == L.ESPACE:
        buf = ctx.alloc(16 * r.count + 64)
        r = ctx.download_plan(*args, buf.ptr, r.count)
    if r.status == L.EFORMAT:
        if buf is not None:
            buf.free()
        return _err(r.err, r.err_part)
    if r.status != L.OK:
        raise RuntimeError(f"shockidx_download_plan: {r.status} {r.err!r}")
    return Streamer(DeviceSections(buf, r.count), Filter, Size=_go_i64(r.size)), None


def Download(node_type: str, idx_name: str, idx_type: str, total_units: int, idx_path: str, parts=None,  # noqa: N802
             file_size: int = 0, chunk_size: int | None = None, record_total_units: int | None = None,
             record_idx_path: str | None = None, Filter: str | None = None):  # noqa: N803
    """single.go:343-484.  parts None: the query has no `part`.  idx_type: IdxInfo.Type, "virtual" for
    the size index.  record_total_units None: the node has no record index (n.Indexes["record"])."""
    has_part = parts is not None
    if idx_type == "virtual":  # :350-367
        if node_type == "subset":
            return _err(E_VIRTUAL_SUBSET)
        csize = CHUNK_SIZE if chunk_size is None else int(chunk_size)
    if node_type == "subset" and idx_name == "chunkrecord":  # :373-431
        if record_total_units is None:
            return _err(E_RECORD_INDEX)
        if not has_part:  # the full subset file: one Range over the record index (:388-400)
            return _plan(L.PLAN_RANGE, [f"1-{record_total_units}"], record_idx_path, record_total_units, Filter=Filter)
        return _plan(L.PLAN_CHUNK_RANGE, parts, idx_path, total_units, record_idx_path, record_total_units,
                     Filter=Filter)
    if not has_part and idx_type == "subset":  # :433-445
        return _plan(L.PLAN_RANGE, [f"1-{total_units}"], idx_path, total_units, Filter=Filter)
    if not has_part:  # :477-482
        return _err(E_NEEDS_PART)
    if idx_type == "subset":  # :450-460
        return _plan(L.PLAN_RANGE, parts, idx_path, total_units, Filter=Filter)
    if len(parts) and file_size == 0:  # :462-466 an empty node has no parts
        return _err(E_INDEX_OUT_BOUNDS, 0)
    if idx_type == "virtual":  # idx.Part is SizePart (virtual.go:46-48)
        return _plan(L.PLAN_SIZE, parts, file_size=file_size, chunk_size=csize, Filter=Filter)
    return _plan(L.PLAN_PART, parts, idx_path, total_units, Filter=Filter)  # :467-474
