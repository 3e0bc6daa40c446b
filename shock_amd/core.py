"""Python host API over libshockidx (product path; no CPU fallback)."""
from __future__ import annotations

import ctypes
import os
import weakref
from dataclasses import dataclass, field

import numpy as np

from . import _lib as L


@dataclass
class IndexResult:
    count: int
    fmt: str | None
    status: int
    err: bytes | None
    rows: np.ndarray | None = None  # uint64 [count, 2] {offset, length}
    timings: dict = field(default_factory=dict)
    path: int = 0  # 1: tile pass, 2: two-pass build, 3: slab-pipelined host build (diagnostic)
    reruns: int = 0
    state_out: int = 0
    term_code: int = 0
    flags: int = 0
    fixups: int = 0
    fix_tiles: int = 0
    row_off: int = 0  # batch builds: the node's first row in the batch's table

    @property
    def ok(self) -> bool:
        return self.status == L.OK


@dataclass
class BatchResult:
    """One batch build: the call's status (system errors only), the nodes with status OK, the table's
    extent in rows (with ESPACE: a capacity with which the call succeeds) and one IndexResult per node."""
    status: int
    count: int
    rows_total: int
    items: list
    err: bytes | None = None
    timings: dict = field(default_factory=dict)

    @property
    def ok(self) -> bool:
        return self.status == L.OK


def _kind(kind) -> int:
    if kind in ("record", L.RECORD):
        return L.RECORD
    if kind in ("line", L.LINE):
        return L.LINE
    raise ValueError(f"unknown index kind {kind!r}")


def _fmt(fmt) -> int:
    if isinstance(fmt, int):
        return fmt
    return L.FMT_CODES[fmt]


def _result(res: L.Result, rc: int, rows=None) -> IndexResult:
    if rc < 0 and rc not in (L.EINVAL, L.ESPACE):
        raise L.ShockIdxError(rc, bytes(res.err)[:res.err_len].decode("utf-8", "replace"))
    msg = ctypes.string_at(ctypes.addressof(res) + L.Result.err.offset, res.err_len)
    return IndexResult(count=int(res.count), fmt=L.FMT_NAMES.get(res.format), status=rc,
                       err=msg if rc != L.OK else None, rows=rows,
                       timings={"kernel_ms": res.kernel_ms, "h2d_ms": res.h2d_ms, "d2h_ms": res.d2h_ms,
                                "total_ms": res.total_ms, "index_ms": res.index_ms},
                       path=int(res.path), reruns=int(res.reruns),
                       state_out=int(res.state_out), term_code=int(res.term_code), flags=int(res.flags),
                       fixups=int(res.fixups), fix_tiles=int(res.fix_tiles))


def _take_rows(ptr, count: int) -> np.ndarray:
    """The library's malloc'ed table as an array without a copy (freed with the array)."""
    lib = L.lib()
    if count == 0:
        lib.shockidx_free(ctypes.cast(ptr, ctypes.c_void_p))
        return np.zeros((0, 2), dtype=np.uint64)
    flat = np.ctypeslib.as_array(ptr, shape=(count * 2,))
    weakref.finalize(flat, lib.shockidx_free, ctypes.cast(ptr, ctypes.c_void_p).value)
    return flat.reshape(count, 2)


class Context:
    """One libshockidx context (HIP stream + workspaces) bound to a device."""

    def __init__(self, device: int = 0):
        self._lib = L.lib()
        h = ctypes.c_void_p()
        rc = self._lib.shockidx_ctx_create(device, ctypes.byref(h))
        if rc != L.OK:
            raise L.ShockIdxError(rc, f"shockidx_ctx_create(device={device}) failed "
                                      f"({self._lib.shockidx_strerror(rc).decode()})")
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.shockidx_ctx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- host-memory build (POSTed body buffer) ------------------------------------------
    def build_host(self, data, kind="record", fmt=None) -> IndexResult:
        if isinstance(data, np.ndarray):
            buf = np.ascontiguousarray(data, dtype=np.uint8)
        else:
            buf = np.frombuffer(bytes(data), dtype=np.uint8)
        ptr = buf.ctypes.data if buf.size else None
        res = L.Result()
        rows_p = ctypes.POINTER(ctypes.c_uint64)()
        rc = self._lib.shockidx_build_host(self._h, ptr, buf.size, _kind(kind), _fmt(fmt),
                                           ctypes.byref(rows_p), ctypes.byref(res))
        rows = _take_rows(rows_p, int(res.count)) if rows_p else None
        return _result(res, rc, rows)

    def host_register(self, buf: np.ndarray) -> None:
        """Pin a host array for direct DMA (shockidx_host_register); build_host on it then
        skips the staging copy.  Undo with host_unregister before the array is freed."""
        rc = self._lib.shockidx_host_register(self._h, buf.ctypes.data, buf.nbytes)
        if rc != 0:
            raise RuntimeError(f"shockidx_host_register failed ({rc})")

    def host_unregister(self, buf: np.ndarray) -> None:
        rc = self._lib.shockidx_host_unregister(self._h, buf.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"shockidx_host_unregister failed ({rc})")

    # -- file build ------------------------------------------------------------------------
    def build_fd(self, fd: int, size: int, kind="record", fmt=None) -> IndexResult:
        res = L.Result()
        rows_p = ctypes.POINTER(ctypes.c_uint64)()
        rc = self._lib.shockidx_build_fd(self._h, fd, size, _kind(kind), _fmt(fmt),
                                         ctypes.byref(rows_p), ctypes.byref(res))
        rows = _take_rows(rows_p, int(res.count)) if rows_p else None
        return _result(res, rc, rows)

    def create(self, fd: int, size: int, kind, tmpdir: str, outpath: str) -> IndexResult:
        res = L.Result()
        rc = self._lib.shockidx_create(self._h, fd, size, _kind(kind), os.fsencode(tmpdir),
                                       os.fsencode(outpath), ctypes.byref(res))
        return _result(res, rc)

    # -- device-resident build ---------------------------------------------------------------
    def build_device(self, d_data: int, n: int, d_rows: int, row_cap: int, kind="record", fmt=None,
                     stream: int | None = None) -> IndexResult:
        """d_data / d_rows are device pointers (e.g. torch tensor .data_ptr())."""
        res = L.Result()
        rc = self._lib.shockidx_build_device(self._h, d_data, n, _kind(kind), _fmt(fmt), d_rows, row_cap,
                                             stream, ctypes.byref(res))
        return _result(res, rc)

    def build_buffer(self, data: "DeviceBuffer", n: int, rows: "DeviceBuffer", kind="record", fmt=None,
                     stream: int | None = None) -> IndexResult:
        """Device-resident build over DeviceBuffers (rows capacity = rows.nbytes // 16)."""
        return self.build_device(data.ptr, n, rows.ptr, rows.nbytes // 16, kind, fmt, stream)

    # -- batch build: many small nodes in one device call -----------------------------------
    def _batch_items(self, items, nnodes, d_data, nodes, table=None):
        """shockidx_batch_item[] -> IndexResults; err through shockidx_batch_error for failed nodes only
        (nodes: int64 [nnodes, 2] {pos, len} on the host; d_data None: the context's packed arena)."""
        out = []
        buf = ctypes.create_string_buffer(256)
        for i in range(nnodes):
            it = items[i]
            err = None
            if it.status != L.OK:
                n = ctypes.c_uint64(0)
                rc = self._lib.shockidx_batch_error(self._h, d_data, ctypes.byref(it), nodes[i].ctypes.data, buf, 255,
                                                    ctypes.byref(n))
                if rc != L.OK:
                    raise L.ShockIdxError(rc, "shockidx_batch_error")
                err = buf.raw[:n.value]
            rows = None
            if table is not None:
                rows = table[int(it.row_off):int(it.row_off) + int(it.count)]
            out.append(IndexResult(count=int(it.count), fmt=L.FMT_NAMES.get(it.format), status=int(it.status), err=err,
                                   rows=rows, path=int(it.path), term_code=int(it.term_code), row_off=int(it.row_off)))
        return out

    def build_batch_device(self, d_data: int, data_len: int, d_nodes: int, nnodes: int, d_rows: int, row_cap: int,
                           kind="record", fmt=None) -> BatchResult:
        """nnodes nodes {int64 pos, int64 len} (d_nodes) of the arena d_data, both in HBM, indexed in one
        call: items[i] is what build_device gives over node i's bytes alone, its rows at
        d_rows[row_off .. row_off + count).  A short row_cap returns ESPACE with rows_total = the
        capacity needed and nothing written; a bad list returns EINVAL."""
        res = L.Result()
        items = (L.BatchItem * max(nnodes, 1))()
        total = ctypes.c_uint64(0)
        rc = self._lib.shockidx_build_batch_device(self._h, d_data, data_len, d_nodes, nnodes, _kind(kind), _fmt(fmt),
                                                   d_rows, row_cap, items, ctypes.byref(total), ctypes.byref(res))
        r = _result(res, rc)
        out = []
        if rc == L.OK and nnodes:
            nodes = np.zeros((nnodes, 2), dtype=np.int64)
            rc2 = self._lib.shockidx_memcpy_d2h(self._h, nodes.ctypes.data, d_nodes, nodes.nbytes)
            if rc2 != L.OK:
                raise L.ShockIdxError(rc2, "shockidx_memcpy_d2h")
            out = self._batch_items(items, nnodes, d_data, nodes)
        return BatchResult(status=rc, count=r.count, rows_total=int(total.value), items=out, err=r.err,
                           timings=r.timings)

    def build_batch_host(self, bodies, kind="record", fmt=None) -> list:
        """One IndexResult per body (bytes-like), each with its own rows view, count, format and status,
        from one device call over all of them (shockidx_build_batch_host)."""
        bufs = [np.frombuffer(bytes(b), dtype=np.uint8) for b in bodies]
        K = len(bufs)
        ptrs = (ctypes.c_void_p * max(K, 1))(*[b.ctypes.data if b.size else None for b in bufs])
        lens = (ctypes.c_uint64 * max(K, 1))(*[b.size for b in bufs])
        items = (L.BatchItem * max(K, 1))()
        res = L.Result()
        rows_p = ctypes.POINTER(ctypes.c_uint64)()
        rc = self._lib.shockidx_build_batch_host(self._h, ptrs, lens, K, _kind(kind), _fmt(fmt), ctypes.byref(rows_p),
                                                 items, ctypes.byref(res))
        if rc != L.OK:
            if rows_p:
                self._lib.shockidx_free(ctypes.cast(rows_p, ctypes.c_void_p))
            raise L.ShockIdxError(rc, bytes(res.err)[:res.err_len].decode("utf-8", "replace"))
        total = max([int(items[i].row_off) + int(items[i].count) for i in range(K)], default=0)
        table = _take_rows(rows_p, total)
        nodes = np.zeros((max(K, 1), 2), dtype=np.int64)
        pos = 0
        for i, b in enumerate(bufs):  # the packed arena: each body at the next 16-byte boundary
            nodes[i] = (pos, b.size)
            pos = (pos + b.size + 15) & ~15
        return self._batch_items(items, K, None, nodes, table)

    def batch_stats(self) -> dict:
        """How the last batch call ran (shockidx_batch_last_stats): nodes, batches, batched, singles,
        by_format (nodes indexed as FASTQ, FASTA, SAM, line), and the kernel launches and host waits it made."""
        st = L.BatchStats()
        rc = self._lib.shockidx_batch_last_stats(self._h, ctypes.byref(st))
        if rc != L.OK:
            raise L.ShockIdxError(rc, "shockidx_batch_last_stats")
        return {"nodes": int(st.nodes), "batches": int(st.batches), "batched": int(st.batched),
                "singles": int(st.singles), "by_format": [int(v) for v in st.by_format],
                "launches": int(st.launches), "waits": int(st.waits)}

    def chunkrecord_device(self, d_data: int, n: int, d_rows: int, row_cap: int, fmt=None, chunk: int = 0) -> IndexResult:
        """chunkRecord.Create (index/chunkrecord.go:41-99) over device memory; chunk 0 = 1 MiB."""
        res = L.Result()
        rc = self._lib.shockidx_chunkrecord_device(self._h, d_data, n, _fmt(fmt), chunk, d_rows, row_cap,
                                                   ctypes.byref(res))
        return _result(res, rc)

    def chunkrecord_fd(self, fd: int, size: int, fmt=None, chunk: int = 0) -> IndexResult:
        """chunkRecord.Create over an open file (shockidx_chunkrecord_fd); rows on the host."""
        res = L.Result()
        rows_p = ctypes.POINTER(ctypes.c_uint64)()
        rc = self._lib.shockidx_chunkrecord_fd(self._h, fd, size, _fmt(fmt), chunk, ctypes.byref(rows_p),
                                               ctypes.byref(res))
        rows = _take_rows(rows_p, int(res.count)) if rows_p else None
        return _result(res, rc, rows)

    def chunkrecord_subset_device(self, d_ri: int, nrows: int, d_rows: int, row_cap: int) -> IndexResult:
        """chunkRecord.Create for a subset node (index/chunkrecord.go:100-228) over its device-
        resident record index (nrows rows); rows (16 * first row, 16 * rows)."""
        res = L.Result()
        rc = self._lib.shockidx_chunkrecord_subset_device(self._h, d_ri, nrows, d_rows, row_cap, ctypes.byref(res))
        return _result(res, rc, None)

    def chunkrecord_subset(self, ri: np.ndarray) -> IndexResult:
        """The same from a host record index (uint64[k, 2]); the rows come back on the host."""
        ri = np.ascontiguousarray(ri, dtype=np.uint64).reshape(-1, 2)
        k = len(ri)
        src = self.alloc(16 * k + 16)
        out = self.alloc(16 * k + 16)
        try:
            if k:
                src.upload(ri.view(np.uint8).reshape(-1))
            r = self.chunkrecord_subset_device(src.ptr, k, out.ptr, max(k, 1))
            if r.status == L.OK:
                r.rows = out.rows(r.count) if r.count else np.zeros((0, 2), np.uint64)
            return r
        finally:
            src.free()
            out.free()

    def chunkrecord_buffer(self, data: "DeviceBuffer", n: int, rows: "DeviceBuffer", fmt=None,
                           chunk: int = 0) -> IndexResult:
        return self.chunkrecord_device(data.ptr, n, rows.ptr, rows.nbytes // 16, fmt, chunk)

    @staticmethod
    def chunkrecord_capacity(n: int, chunk: int = 0) -> int:
        """Rows a chunkrecord build can produce (include/shockidx.h)."""
        return n // ((chunk or 1048576) - 32767) + 2

    # -- chunkrecord in slabs (shockidx_chunkrecord_slab_device and the walk over it) ------------
    def chunkrecord_carry(self) -> "DeviceBuffer":
        """Device memory for the carry of one chunkrecord slab walk (shockidx_chunkrecord_carry_bytes;
        the first slab initialises it)."""
        return self.alloc(int(self._lib.shockidx_chunkrecord_carry_bytes()))

    def chunkrecord_slab(self, buf: "DeviceBuffer", base: int, front: int, end: int, file_size: int,
                         carry: "DeviceBuffer", rows: "DeviceBuffer", fmt=None, chunk: int = 0, first=None,
                         last=None) -> IndexResult:
        """One slab of chunkrecord over the file bytes [base - front, base + end), where buf holds the
        file from offset 0 (so base must be a multiple of 16).  Slabs go in file order with the carry
        between them on the device.  OK: count rows at file offsets in rows (possibly 0); ESPACE: count
        = the rows the slab needs; EINVAL: the carry's next window starts before the slab's window.
        Anything but OK leaves the carry untouched.  first / last default to what the window says."""
        slab = L.Slab(d_data=buf.ptr + base, n=end, end=end, front=front, base=base,
                      is_first=int(front == base if first is None else first),
                      is_last=int(base + end == file_size if last is None else last), seq=0, reserved=0)
        res = L.Result()
        rc = self._lib.shockidx_chunkrecord_slab_device(self._h, ctypes.byref(slab), file_size, _fmt(fmt), chunk,
                                                        carry.ptr, rows.ptr, rows.nbytes // 16, ctypes.byref(res))
        return _result(res, rc)

    def chunkrecord_fd_walk(self, fd: int, size: int, fmt=None, chunk: int = 0, slab_bytes: int = 0) -> IndexResult:
        """chunkRecord.Create over an open file, always slab by slab (shockidx_chunkrecord_fd_walk; 0:
        slabs sized to the device budget); rows on the host, path 6."""
        res = L.Result()
        rows_p = ctypes.POINTER(ctypes.c_uint64)()
        rc = self._lib.shockidx_chunkrecord_fd_walk(self._h, fd, size, _fmt(fmt), chunk, slab_bytes,
                                                    ctypes.byref(rows_p), ctypes.byref(res))
        rows = _take_rows(rows_p, int(res.count)) if rows_p else None
        return _result(res, rc, rows)

    # -- column index (index/column.go:33-130) ---------------------------------------------------
    def column_device(self, d_data: int, n: int, column: int, d_rows: int, row_cap: int) -> IndexResult:
        """CreateColumnIndex over device memory: rows of the runs of the column-th tab-separated
        field (column counts from 1).  EFORMAT carries Go's "Specified column does not exist ..."."""
        res = L.Result()
        rc = self._lib.shockidx_column_device(self._h, d_data, n, column, d_rows, row_cap, ctypes.byref(res))
        return _result(res, rc)

    def column_buffer(self, data: "DeviceBuffer", n: int, column: int, rows: "DeviceBuffer") -> IndexResult:
        return self.column_device(data.ptr, n, column, rows.ptr, rows.nbytes // 16)

    def column_fd(self, fd: int, size: int, column: int) -> IndexResult:
        """CreateColumnIndex over an open file (shockidx_column_fd); rows on the host."""
        res = L.Result()
        rows_p = ctypes.POINTER(ctypes.c_uint64)()
        rc = self._lib.shockidx_column_fd(self._h, fd, size, column, ctypes.byref(rows_p), ctypes.byref(res))
        rows = _take_rows(rows_p, int(res.count)) if rows_p else None
        return _result(res, rc, rows)

    def column_host(self, data, column: int) -> IndexResult:
        """Host-memory convenience: upload, build on the device, download the rows."""
        data = bytes(data)
        n = len(data)
        d_in = self.alloc(n + 64)
        d_in.upload(data)
        cap = 1024
        d_rows = self.alloc(16 * cap)
        try:
            r = self.column_buffer(d_in, n, column, d_rows)
            if r.status == L.ESPACE:  # r.count holds the rows needed
                d_rows.free()
                cap = r.count
                d_rows = self.alloc(16 * cap)
                r = self.column_buffer(d_in, n, column, d_rows)
            if r.status == L.OK:
                r.rows = d_rows.rows(r.count) if r.count else np.zeros((0, 2), np.uint64)
            return r
        finally:
            d_in.free()
            d_rows.free()

    # -- column index in slabs (shockidx_column_slab_device and the walk over it) -----------------
    def column_carry(self) -> "DeviceBuffer":
        """Device memory for the carry of one slab walk (shockidx_column_carry_bytes; the first slab
        initialises it)."""
        return self.alloc(int(self._lib.shockidx_column_carry_bytes()))

    def column_slab(self, slab: "L.Slab", file_size: int, column: int, d_carry: int, d_rows: int,
                    row_cap: int) -> IndexResult:
        """One slab of the column index (slabs go in file order, the carry between them on the device).
        OK: count rows at file offsets in d_rows; ESPACE: count = the rows the slab needs; EFORMAT: the
        missing-column error; EMORE: state_out = the file offset of the first owned line the slab's
        window cannot settle.  Anything but OK leaves the carry untouched."""
        res = L.Result()
        rc = self._lib.shockidx_column_slab_device(self._h, ctypes.byref(slab), file_size, column, d_carry, d_rows,
                                                   row_cap, ctypes.byref(res))
        return _result(res, rc)

    def column_fd_walk(self, fd: int, size: int, column: int, slab_bytes: int = 0, halo_bytes: int = 0) -> IndexResult:
        """CreateColumnIndex over an open file, always slab by slab (shockidx_column_fd_walk; 0: slabs
        sized to the device budget, a 4 MiB halo); rows on the host, path 5."""
        res = L.Result()
        rows_p = ctypes.POINTER(ctypes.c_uint64)()
        rc = self._lib.shockidx_column_fd_walk(self._h, fd, size, column, slab_bytes, halo_bytes, ctypes.byref(rows_p),
                                               ctypes.byref(res))
        rows = _take_rows(rows_p, int(res.count)) if rows_p else None
        return _result(res, rc, rows)

    def column_create(self, fd: int, size: int, column: int, tmpdir: str, outpath: str) -> IndexResult:
        """CreateColumnIndex with its file protocol (shockidx_column_create): the table through a temp
        file under tmpdir to outpath; on an error neither is left behind."""
        res = L.Result()
        rc = self._lib.shockidx_column_create(self._h, fd, size, column, os.fsencode(tmpdir), os.fsencode(outpath),
                                              ctypes.byref(res))
        return _result(res, rc)

    def set_dev_cap(self, nbytes: int) -> None:
        """Device bytes one fd build may hold (shockidx_ctx_set_dev_cap; 0: what is free).  A node
        whose one-pass build would not fit is indexed through two slab slots sized to the cap."""
        rc = self._lib.shockidx_ctx_set_dev_cap(self._h, int(nbytes))
        if rc != 0:
            raise L.ShockIdxError(rc, "shockidx_ctx_set_dev_cap failed")

    def trim(self, keep_bytes: int = 0) -> None:
        """Free the context's cached device workspaces down to keep_bytes (shockidx_ctx_trim)."""
        rc = self._lib.shockidx_ctx_trim(self._h, int(keep_bytes))
        if rc != L.OK:
            raise L.ShockIdxError(rc, "shockidx_ctx_trim failed")

    def debug_set_tiles_grid(self, g: int) -> None:
        """Debug entry (shockidx_debug_set_tiles_grid, not in the public header): run every tile pass on
        at most g workgroups, so a test reaches the edges of the claim plan with a few MiB.  Only before
        the context's first build."""
        fn = self._lib.shockidx_debug_set_tiles_grid  # (bound here: a variant library of older sources has none)
        fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_int], ctypes.c_int
        rc = fn(self._h, int(g))
        if rc != L.OK:
            raise L.ShockIdxError(rc, "shockidx_debug_set_tiles_grid failed (after the first build, or g out of range)")

    def workspace_bytes(self) -> int:
        return int(self._lib.shockidx_ctx_workspace_bytes(self._h))

    def alloc(self, nbytes: int, node: bool = False) -> "DeviceBuffer":
        """node=True: a node body the index streams (shockidx_dev_alloc_node: contiguous HBM)."""
        return DeviceBuffer(self, nbytes, node)

    def sync(self):
        rc = self._lib.shockidx_sync(self._h)
        if rc != L.OK:
            raise L.ShockIdxError(rc, "shockidx_sync failed")

    @property
    def stream(self) -> int:
        return self._lib.shockidx_stream(self._h)

    # -- subset nodes (index/subset.go:133-303) -------------------------------------------------
    def subset_index(self, d_ids: int, ids_len: int, d_parent: int, parent_count: int, ilength: int, d_rows: int,
                     rows_cap: int, d_runs: int, runs_cap: int) -> SubsetResult:
        r = L.SubsetResult()
        rc = self._lib.shockidx_subset_index(self._h, d_ids, ids_len, d_parent, parent_count, ilength, d_rows, rows_cap,
                                             d_runs, runs_cap, ctypes.byref(r))
        return _sub_result(r, rc)

    def subset_gather(self, d_data: int, data_len: int, d_runs: int, nruns: int, d_out: int,
                      out_cap: int) -> SubsetResult:
        r = L.SubsetResult()
        rc = self._lib.shockidx_subset_gather(self._h, d_data, data_len, d_runs, nruns, d_out, out_cap,
                                              ctypes.byref(r))
        return _sub_result(r, rc)

    def subset_node(self, d_ids: int, ids_len: int, d_parent: int, parent_count: int, ilength: int, d_rows: int,
                    rows_cap: int, d_runs: int, runs_cap: int, d_data: int, data_len: int, d_out: int,
                    out_cap: int) -> SubsetResult:
        """subset_index + subset_gather in one call (the counts between them stay on the device)."""
        r = L.SubsetResult()
        rc = self._lib.shockidx_subset_node(self._h, d_ids, ids_len, d_parent, parent_count, ilength, d_rows, rows_cap,
                                            d_runs, runs_cap, d_data, data_len, d_out, out_cap, ctypes.byref(r))
        return _sub_result(r, rc)

    def subset_host(self, ids, parent_rows, ilength=None, data=None) -> SubsetResult:
        """Host-memory convenience: upload the id text and the parent rows, build the subset
        index on the device, download rows + runs (and the gathered bytes when `data` is given)."""
        ids = bytes(ids)
        par = np.ascontiguousarray(parent_rows, dtype=np.uint64).reshape(-1, 2)
        n = par.shape[0]
        il = n if ilength is None else int(ilength)
        d_ids = self.alloc(len(ids) + 64)
        d_ids.upload(ids)
        d_par = self.alloc(16 * n + 64)
        if n:
            d_par.upload(par.tobytes())
        cap = max(1, len(ids) // 2 + 2)
        d_rows = self.alloc(16 * cap)
        d_runs = self.alloc(16 * cap)
        r = self.subset_index(d_ids.ptr, len(ids), d_par.ptr, n, il, d_rows.ptr, cap, d_runs.ptr, cap)
        if r.status in (L.OK, L.EFORMAT):
            r.rows = d_rows.rows(r.count) if r.count else np.zeros((0, 2), np.uint64)
            nr = r.runs if r.ok else 0
            r.run_rows = d_runs.rows(nr) if nr else np.zeros((0, 2), np.uint64)
        if data is not None and r.ok:
            d_data = self.alloc(len(data) + 64)
            d_data.upload(bytes(data))
            d_out = self.alloc(max(r.size, 1) + 64)
            g = self.subset_gather(d_data.ptr, len(data), d_runs.ptr, r.runs, d_out.ptr, max(r.size, 1))
            r.gathered = d_out.download(g.size).tobytes() if g.ok else None
            d_data.free()
            d_out.free()
        for b in (d_ids, d_par, d_rows, d_runs):
            b.free()
        return r

    def create_subset_index(self, d_ids: int, ids_len: int, d_parent: int, parent_count: int, ilength: int,
                            d_rows: int, rows_cap: int) -> SubsetResult:
        """subset.go:36-128 CreateSubsetIndex on device memory (count = size = 2**64-1 on error)."""
        r = L.SubsetResult()
        rc = self._lib.shockidx_create_subset_index(self._h, d_ids, ids_len, d_parent, parent_count, ilength, d_rows,
                                                    rows_cap, ctypes.byref(r))
        return _sub_result(r, rc)

    # -- subset indexes in slabs and from files (shockidx_subset_slab_device and the walk over it) --
    def subset_carry(self) -> "DeviceBuffer":
        """Zeroed device memory for the carry of one subset walk (shockidx_subset_carry_bytes; the first
        slab initialises it)."""
        b = self.alloc(int(self._lib.shockidx_subset_carry_bytes()))
        b.upload(bytes(b.nbytes))
        return b

    def subset_slab(self, slab: "L.Slab", ids_size: int, d_parent: int, prow0: int, prows: int, parent_count: int,
                    ilength: int, want_runs: bool, d_carry: int, d_rows: int, rows_cap: int, d_runs: int,
                    runs_cap: int) -> "L.SubsetSlabResult":
        """One slab of the id text against one window of the parent index (slabs in file order, the loop's
        state in the device carry).  Returns the raw result: status OK (rows / runs written, the running
        totals, stop and next_off / next_id), EFORMAT (Go's text; the walk has ended), ESPACE (rows / runs
        = what the call needs; the carry is unchanged) or EINVAL."""
        res = L.SubsetSlabResult()
        rc = self._lib.shockidx_subset_slab_device(self._h, ctypes.byref(slab), ids_size, d_parent, prow0, prows,
                                                   parent_count, int(ilength), 1 if want_runs else 0, d_carry, d_rows,
                                                   rows_cap, d_runs, runs_cap, ctypes.byref(res))
        if rc < 0 and rc not in (L.EINVAL, L.ESPACE):
            raise L.ShockIdxError(rc, res.message.decode("utf-8", "replace"))
        res.status = rc
        return res

    def subset_fd_walk(self, ids_fd: int, ids_size: int, parent_fd: int, parent_bytes: int, ilength: int,
                       want_runs: bool = True, ids_slab_bytes: int = 0, parent_slab_rows: int = 0) -> SubsetResult:
        """The subset builders over two open files, always slab by slab (shockidx_subset_fd_walk; 0: sized
        to the device budget); rows and run_rows on the host (on EFORMAT: what was written before it)."""
        r = L.SubsetResult()
        rows_p, runs_p = ctypes.POINTER(ctypes.c_uint64)(), ctypes.POINTER(ctypes.c_uint64)()
        rc = self._lib.shockidx_subset_fd_walk(self._h, ids_fd, ids_size, parent_fd, parent_bytes, int(ilength),
                                               1 if want_runs else 0, ids_slab_bytes, parent_slab_rows,
                                               ctypes.byref(rows_p), ctypes.byref(runs_p) if want_runs else None,
                                               ctypes.byref(r))
        out = _sub_result(r, rc)
        if rows_p:
            out.rows = _take_rows(rows_p, out.count)
        if runs_p:
            out.run_rows = _take_rows(runs_p, out.runs)
        return out

    def subset_create(self, ids_fd: int, ids_size: int, parent_fd: int, parent_bytes: int, ilength: int, tmpdir: str,
                      cofile, ofile: str) -> SubsetResult:
        """CreateSubsetNodeIndexes with its file protocol (shockidx_subset_create), CreateSubsetIndex's with
        cofile None: the tables through temp files under tmpdir, cofile renamed first, then ofile; on an
        error nothing is left behind."""
        r = L.SubsetResult()
        rc = self._lib.shockidx_subset_create(self._h, ids_fd, ids_size, parent_fd, parent_bytes, int(ilength),
                                              os.fsencode(tmpdir), os.fsencode(cofile) if cofile is not None else None,
                                              os.fsencode(ofile), ctypes.byref(r))
        return _sub_result(r, rc)

    def subset_stats(self) -> dict:
        """How the last subset_fd_walk / subset_create ran (shockidx_subset_last_stats)."""
        st = L.SubsetStats()
        rc = self._lib.shockidx_subset_last_stats(self._h, ctypes.byref(st))
        if rc != L.OK:
            raise L.ShockIdxError(rc, "shockidx_subset_last_stats")
        return {k: int(getattr(st, k)) for k, _ in L.SubsetStats._fields_}

    # -- index read path (index/index.go:67-193) ---------------------------------------------------
    def idx_part(self, d_rows, nrows: int, part: str, idx_length: int):
        """Idx.Part over a device-resident index (d_rows None: the file is missing).
        Returns (pos, length, err bytes|None)."""
        r = L.SubsetResult()
        pos, length = ctypes.c_int64(0), ctypes.c_int64(0)
        rc = self._lib.shockidx_idx_part(self._h, d_rows, nrows, part.encode(), int(idx_length), ctypes.byref(pos),
                                         ctypes.byref(length), ctypes.byref(r))
        if rc == L.EFORMAT:
            return 0, 0, r.message
        if rc != L.OK:
            raise RuntimeError(f"shockidx_idx_part: {rc} {r.message!r}")
        return pos.value, length.value, None

    def idx_range(self, d_rows, nrows: int, part: str, idx_length: int, d_recs=None, recs_cap: int = 0):
        """Idx.Range over a device-resident index.  With d_recs the records stay on the device
        (returns (count, None)); without, they are returned as int64[k, 2].  Returns (recs|count, err|None)."""
        r = L.SubsetResult()
        own = None
        if d_recs is None:  # size the output with a first call
            rc = self._lib.shockidx_idx_range(self._h, d_rows, nrows, part.encode(), int(idx_length), None, 0,
                                              ctypes.byref(r))
            if rc == L.EFORMAT:
                return np.zeros((0, 2), np.int64), r.message
            if rc not in (L.OK, L.ESPACE):  # ESPACE: r.count holds the records needed
                raise RuntimeError(f"shockidx_idx_range: {rc} {r.message!r}")
            recs_cap = max(int(r.count), 1)
            own = self.alloc(16 * recs_cap + 64)
            d_recs = own.ptr
        rc = self._lib.shockidx_idx_range(self._h, d_rows, nrows, part.encode(), int(idx_length), d_recs, recs_cap,
                                          ctypes.byref(r))
        if rc == L.EFORMAT:
            if own is not None:
                own.free()
            return (np.zeros((0, 2), np.int64) if own is not None else 0), r.message
        if rc != L.OK:
            raise RuntimeError(f"shockidx_idx_range: {rc} {r.message!r}")
        if own is None:
            return int(r.count), None
        out = own.rows(int(r.count)).view(np.int64) if r.count else np.zeros((0, 2), np.int64)
        own.free()
        return out, None

    # -- download filters (node/filter/) -------------------------------------------------------
    def filter_device(self, name: str, d_data: int, n: int, d_out: int, out_cap: int) -> SubsetResult:
        """fq2fa over a FASTQ section, anonymize over a FASTQ, FASTA or SAM section (the format is
        detected first) in HBM (count = records, size = bytes out; ESPACE: size = the bytes needed)."""
        r = L.SubsetResult()
        rc = self._lib.shockidx_filter_device(self._h, name.encode(), d_data, n, d_out, out_cap, ctypes.byref(r))
        return _sub_result(r, rc)

    def filter_host(self, name: str, data) -> SubsetResult:
        """Host-memory convenience: upload, filter on the device, download (r.gathered = bytes)."""
        data = bytes(data)
        d_in = self.alloc(len(data) + 64)
        d_in.upload(data)
        cap = 2 * len(data) + 64  # anonymize may lengthen short records (counter digits)
        d_out = self.alloc(cap)
        try:
            r = self.filter_device(name, d_in.ptr, len(data), d_out.ptr, cap)
            if r.status == L.ESPACE:  # many tiny FASTA records: r.size holds the bytes needed
                d_out.free()
                cap = int(r.size) + 64
                d_out = self.alloc(cap)
                r = self.filter_device(name, d_in.ptr, len(data), d_out.ptr, cap)
            if r.status in (L.OK, L.EFORMAT):
                r.gathered = d_out.download(r.size).tobytes() if r.size else b""
        finally:
            d_in.free()
            d_out.free()
        return r

    # -- the download filters in slabs (shockidx_filter_slab_device and the walk over it) ----------
    def filter_carry(self) -> "DeviceBuffer":
        """Device memory for the carry of one filter slab walk (shockidx_filter_carry_bytes; the first
        slab initialises it)."""
        return self.alloc(int(self._lib.shockidx_filter_carry_bytes()))

    @staticmethod
    def filter_carry_state(carry: "DeviceBuffer") -> dict:
        """The carry's current half: pos (the next Read's section offset), count, bytes, kind, ended."""
        fc = L.FilterCarry.from_buffer_copy(carry.download(ctypes.sizeof(L.FilterCarry)).tobytes())
        h = fc.half[fc.cur & 1]
        return {"pos": int(h.pos), "count": int(h.count), "bytes": int(h.bytes), "kind": int(h.kind),
                "ended": bool(h.ended)}

    def filter_slab(self, name: str, buf: "DeviceBuffer", base: int, front: int, n: int, end: int, sec_size: int,
                    carry: "DeviceBuffer", out: "DeviceBuffer", first=None, last=None, out_cap=None) -> SubsetResult:
        """One slab of a FASTQ section through fq2fa / anonymize: the window is the section bytes
        [base - front, base + end), n of them owned, where buf holds the section from offset 0 (so base
        must be a multiple of 16).  Slabs go in order with the carry between them on the device.  OK /
        EFORMAT: count records and size bytes in out, r.next_pos the carried position; ESPACE: size =
        the bytes the slab needs; EINVAL: see include/shockidx.h.  Anything but OK or EFORMAT leaves the
        carry untouched.  first / last default to what the window says."""
        slab = L.Slab(d_data=buf.ptr + base, n=n, end=end, front=front, base=base,
                      is_first=int(base - front == 0 if first is None else first),
                      is_last=int(base + end == sec_size if last is None else last), seq=0, reserved=0)
        r = L.SubsetResult()
        pos = ctypes.c_uint64(0)
        rc = self._lib.shockidx_filter_slab_device(self._h, name.encode(), ctypes.byref(slab), sec_size, carry.ptr,
                                                   out.ptr, out.nbytes if out_cap is None else out_cap,
                                                   ctypes.byref(pos), ctypes.byref(r))
        res = _sub_result(r, rc)
        res.next_pos = int(pos.value)
        return res

    def _filter_fd_result(self, r: "L.SubsetResult", rc: int) -> SubsetResult:
        if rc < 0 and rc not in (L.EINVAL, L.ENOMEM, L.EIO):
            raise L.ShockIdxError(rc, r.message.decode("utf-8", "replace"))
        return SubsetResult(count=int(r.count), runs=0, size=int(r.size), status=rc, err=r.message if rc != L.OK else None,
                            kernel_ms=r.kernel_ms, total_ms=r.total_ms, gather_ms=r.gather_ms)

    def filter_fd_walk(self, name: str, fd: int, off: int, n: int, out_fd: int, slab_bytes: int = 0,
                       halo_bytes: int = 0) -> SubsetResult:
        """The section [off, off + n) of fd through fq2fa / anonymize, always slab by slab
        (shockidx_filter_fd_walk; 0: sized to the device budget), the stream written to out_fd (a file, a
        pipe, a socket).  status OK, EFORMAT (Go's text, after the delivered bytes were written), ENOMEM
        (a record no slot can hold), EIO (the write failed) or EINVAL; count / size = what was delivered."""
        r = L.SubsetResult()
        rc = self._lib.shockidx_filter_fd_walk(self._h, name.encode(), fd, off, n, out_fd, slab_bytes, halo_bytes,
                                               ctypes.byref(r))
        return self._filter_fd_result(r, rc)

    def filter_fd(self, name: str, fd: int, off: int, n: int, out_fd: int) -> SubsetResult:
        """The same through shockidx_filter_fd: the whole path when the section, its output and the
        workspace fit the device budget, else the walk (anonymize: FASTQ sections only)."""
        r = L.SubsetResult()
        rc = self._lib.shockidx_filter_fd(self._h, name.encode(), fd, off, n, out_fd, ctypes.byref(r))
        return self._filter_fd_result(r, rc)

    def filter_stats(self) -> dict:
        """How the last filter_fd / filter_fd_walk ran (shockidx_filter_last_stats)."""
        st = L.FilterStats()
        rc = self._lib.shockidx_filter_last_stats(self._h, ctypes.byref(st))
        if rc != L.OK:
            raise L.ShockIdxError(rc, "shockidx_filter_last_stats")
        return {k: int(getattr(st, k)) for k, _ in L.FilterStats._fields_}

    # -- the sectioned stream (request/streamer.go:78-98) -----------------------------------------
    def stream_filter_device(self, name, d_data: int, data_len: int, d_secs: int, nsecs: int, d_out: int,
                             out_cap: int) -> SubsetResult:
        """Streamer.Stream with a Filter over nsecs sections {int64 pos, int64 len} (d_secs, the records
        idx_range leaves on the device) of a node in HBM: every section through its own filter reader,
        the outputs back to back (count = records, size = bytes out).  name None: no filter (the
        gather).  r.err_section: the failing section (Streamer.ESection) or -1."""
        r = L.SubsetResult()
        es = ctypes.c_int64(-1)
        rc = self._lib.shockidx_stream_filter_device(self._h, name.encode() if name else None, d_data, data_len, d_secs,
                                                     nsecs, d_out, out_cap, ctypes.byref(es), ctypes.byref(r))
        out = _sub_result(r, rc)
        out.err_section = int(es.value)
        return out

    def stream_stats(self) -> dict:
        """Which path the last stream_filter_device call with a filter took (shockidx_stream_last_stats):
        sections, batches (groups of small sections of one format that took the segmented path), batched
        (sections inside them), singles (sections through the single-section filter) and by_format
        (batches of FASTQ, FASTA, SAM sections)."""
        st = L.StreamStats()
        rc = self._lib.shockidx_stream_last_stats(self._h, ctypes.byref(st))
        if rc != L.OK:
            raise L.ShockIdxError(rc, "shockidx_stream_last_stats")
        return {"sections": int(st.sections), "batches": int(st.batches), "batched": int(st.batched),
                "singles": int(st.singles), "by_format": [int(v) for v in st.by_format]}

    def stream_filter_host(self, name, data, sections) -> SubsetResult:
        """Host-memory convenience: upload the node and the sections [(pos, len), ...], stream on the
        device, download (r.gathered = the bytes delivered, also before an error)."""
        data = bytes(data)
        secs = np.ascontiguousarray(np.asarray(list(sections), dtype=np.int64).reshape(-1, 2))
        d_in = self.alloc(len(data) + 64)
        d_in.upload(data)
        d_secs = self.alloc(16 * len(secs) + 64)
        if len(secs):
            d_secs.upload(secs.tobytes())
        cap = 2 * int(secs[:, 1].clip(min=0).sum()) + 64 if len(secs) else 64
        d_out = self.alloc(cap)
        try:
            r = self.stream_filter_device(name, d_in.ptr, len(data), d_secs.ptr, len(secs), d_out.ptr, cap)
            if r.status == L.ESPACE:  # r.size holds the bytes needed
                d_out.free()
                cap = int(r.size) + 64
                d_out = self.alloc(cap)
                r = self.stream_filter_device(name, d_in.ptr, len(data), d_secs.ptr, len(secs), d_out.ptr, cap)
            if r.status in (L.OK, L.EFORMAT):
                r.gathered = d_out.download(r.size).tobytes() if r.size else b""
        finally:
            d_in.free()
            d_secs.free()
            d_out.free()
        return r

    # -- the download plan (controller/node/single.go:372-483) ------------------------------------
    def download_plan(self, mode: int, parts, d_rows, nrows: int, idx_length: int, d_rec_rows=None,
                      rec_nrows: int = 0, rec_length: int = 0, file_size: int = 0, chunk_size: int = 0,
                      d_secs=None, secs_cap: int = 0) -> SubsetResult:
        """All parts of an index download as the Streamer's section list, left on the device
        (shockidx_download_plan; mode: L.PLAN_*).  d_secs receives r.count records {int64 pos, int64
        len}, r.size is Go's `size` (read as uint64); an error is EFORMAT with Go's text in r.err and
        the failing part in r.err_part (-1: none); ESPACE: r.count = the sections needed."""
        r = L.SubsetResult()
        ep = ctypes.c_int64(-1)
        arr = (ctypes.c_char_p * max(len(parts), 1))(*[p.encode() if isinstance(p, str) else bytes(p) for p in parts])
        rc = self._lib.shockidx_download_plan(self._h, mode, arr, len(parts), d_rows, nrows, int(idx_length),
                                              d_rec_rows, rec_nrows, int(rec_length), int(file_size),
                                              int(chunk_size), d_secs, secs_cap, ctypes.byref(ep), ctypes.byref(r))
        out = _sub_result(r, rc)
        out.err_part = int(ep.value)
        return out

    def download_plan_host(self, mode: int, parts, rows, idx_length: int, rec_rows=None, rec_length: int = 0,
                           file_size: int = 0, chunk_size: int = 0):
        """Host-memory convenience: upload the index rows (None: the file is missing), plan on the
        device, download.  Returns (secs int64[k, 2], size as Go's int64, err bytes|None, err_part)."""
        bufs = []

        def up(t):
            if t is None:
                return None, 0
            t = np.ascontiguousarray(t).view(np.uint64).reshape(-1, 2)
            b = self.alloc(16 * len(t) + 64)
            bufs.append(b)
            if len(t):
                b.upload(t.tobytes())
            return b.ptr, len(t)

        try:
            d_rows, nrows = up(rows)
            d_rec, rec_nrows = up(rec_rows)
            args = (mode, list(parts), d_rows, nrows, idx_length, d_rec, rec_nrows, rec_length, file_size, chunk_size)
            r = self.download_plan(*args)  # sizes the output: ESPACE carries the sections needed
            if r.status == L.ESPACE:
                out = self.alloc(16 * r.count + 64)
                bufs.append(out)
                r = self.download_plan(*args, out.ptr, r.count)
            if r.status == L.EFORMAT:
                return np.zeros((0, 2), np.int64), 0, r.err, r.err_part
            if r.status != L.OK:
                raise RuntimeError(f"shockidx_download_plan: {r.status} {r.err!r}")
            secs = out.rows(r.count).view(np.int64) if r.count else np.zeros((0, 2), np.int64)
            return secs, _go_i64(r.size), None, -1
        finally:
            for b in bufs:
                b.free()

    def detect(self, data):
        buf = np.frombuffer(bytes(data[:32768]), dtype=np.uint8)
        f = ctypes.c_int(0)
        m = ctypes.c_int(0)
        rc = self._lib.shockidx_detect(self._h, buf.ctypes.data if buf.size else None, buf.size,
                                       ctypes.byref(f), ctypes.byref(m))
        if rc != L.OK:
            raise L.ShockIdxError(rc, "shockidx_detect failed")
        return L.FMT_NAMES.get(f.value), m.value


@dataclass
class SubsetResult:
    count: int        # oCount (rows before an error)
    runs: int         # coCount
    size: int         # oSize
    status: int
    err: bytes | None
    kernel_ms: float = 0.0
    total_ms: float = 0.0
    gather_ms: float = 0.0  # subset_node: device time of the gather
    rows: np.ndarray | None = None
    run_rows: np.ndarray | None = None
    gathered: bytes | None = None
    err_section: int = -1  # stream_filter_device: the failing section (Streamer.ESection)
    err_part: int = -1  # download_plan: the failing part
    next_pos: int = 0  # filter_slab: the carried position (section offset of the next Read)

    @property
    def ok(self) -> bool:
        return self.status == L.OK


def _go_i64(x: int) -> int:
    """a uint64 result word read as Go's int64"""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def _sub_result(r: L.SubsetResult, rc: int) -> SubsetResult:
    if rc < 0 and rc not in (L.EINVAL, L.ESPACE):
        raise L.ShockIdxError(rc, r.message.decode("utf-8", "replace"))
    return SubsetResult(count=int(r.count), runs=int(r.runs), size=int(r.size), status=rc,
                        err=r.message if rc != L.OK else None, kernel_ms=r.kernel_ms, total_ms=r.total_ms,
                        gather_ms=r.gather_ms)


class DeviceBuffer:
    """HBM allocation on a Context's device (libshockidx's HIP runtime; torch's bundled HIP
    runtime is a different library and is not mixed into the same process)."""

    def __init__(self, ctx: Context, nbytes: int, node: bool = False):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        fn = ctx._lib.shockidx_dev_alloc_node if node else ctx._lib.shockidx_dev_alloc
        rc = fn(ctx._h, self.nbytes, ctypes.byref(p))
        if rc != L.OK:
            raise L.ShockIdxError(rc, f"device allocation of {nbytes} bytes failed")
        self.ptr = p.value

    def upload(self, data, offset: int = 0):
        buf = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray)
                                   else data).view(np.uint8).reshape(-1)
        assert offset + buf.size <= self.nbytes
        if buf.size:
            rc = self.ctx._lib.shockidx_memcpy_h2d(self.ctx._h, self.ptr + offset, buf.ctypes.data, buf.size)
            if rc != L.OK:
                raise L.ShockIdxError(rc, "h2d copy failed")

    def download(self, nbytes: int | None = None, offset: int = 0) -> np.ndarray:
        nbytes = self.nbytes - offset if nbytes is None else int(nbytes)
        out = np.empty(nbytes, dtype=np.uint8)
        if nbytes:
            rc = self.ctx._lib.shockidx_memcpy_d2h(self.ctx._h, out.ctypes.data, self.ptr + offset, nbytes)
            if rc != L.OK:
                raise L.ShockIdxError(rc, "d2h copy failed")
        return out

    def rows(self, count: int) -> np.ndarray:
        return self.download(16 * count).view(np.uint64).reshape(count, 2)

    def fill(self, value: int, nbytes: int | None = None, offset: int = 0):
        rc = self.ctx._lib.shockidx_memset(self.ctx._h, self.ptr + offset, value,
                                           self.nbytes - offset if nbytes is None else nbytes)
        if rc != L.OK:
            raise L.ShockIdxError(rc, "memset failed")

    def free(self):
        if self.ptr:
            self.ctx._lib.shockidx_dev_free(self.ctx._h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def write_idx(rows: np.ndarray, tmpdir: str, outpath: str) -> None:
    """The .idx output protocol (record.go:35-41,65-87) through libshockidx."""
    lib = L.lib()
    r = np.ascontiguousarray(rows, dtype=np.uint64)
    err = ctypes.create_string_buffer(256)
    rc = lib.shockidx_write_idx(r.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), r.shape[0],
                                os.fsencode(tmpdir), os.fsencode(outpath), err, 256)
    if rc != L.OK:
        raise L.ShockIdxError(rc, err.value.decode("utf-8", "replace"))


class MultiContext:
    """Several GPUs building one node file from this process (shockidx_multi_*): byte slabs,
    one per device, summaries all-gathered over RCCL (host memory when a device repeats).
    Same results as Context.build_host / build_fd / create."""

    def __init__(self, devices):
        self._lib = L.lib()
        devs = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_void_p()
        rc = self._lib.shockidx_multi_create(devs, len(devices), ctypes.byref(h))
        if rc != L.OK:
            raise L.ShockIdxError(rc, "shockidx_multi_create failed")
        self._h = h
        self.devices = list(devices)
        self._fin = weakref.finalize(self, self._lib.shockidx_multi_destroy, h)

    @property
    def rccl(self) -> bool:
        return bool(self._lib.shockidx_multi_rccl(self._h))

    def close(self):
        self._fin()

    def build_host(self, data, kind="record", fmt=None) -> IndexResult:
        if isinstance(data, np.ndarray):
            buf = np.ascontiguousarray(data, dtype=np.uint8)
        else:
            buf = np.frombuffer(bytes(data), dtype=np.uint8)
        ptr = buf.ctypes.data if buf.size else None
        res = L.Result()
        rows_p = ctypes.POINTER(ctypes.c_uint64)()
        rc = self._lib.shockidx_multi_build_host(self._h, ptr, buf.size, _kind(kind), _fmt(fmt),
                                                 ctypes.byref(rows_p), ctypes.byref(res))
        rows = _take_rows(rows_p, int(res.count)) if rows_p else None
        return _result(res, rc, rows)

    def build_fd(self, fd: int, size: int, kind="record", fmt=None) -> IndexResult:
        res = L.Result()
        rows_p = ctypes.POINTER(ctypes.c_uint64)()
        rc = self._lib.shockidx_multi_build_fd(self._h, fd, size, _kind(kind), _fmt(fmt),
                                               ctypes.byref(rows_p), ctypes.byref(res))
        rows = _take_rows(rows_p, int(res.count)) if rows_p else None
        return _result(res, rc, rows)

    def create(self, fd: int, size: int, kind, tmpdir: str, outpath: str) -> IndexResult:
        res = L.Result()
        rc = self._lib.shockidx_multi_create_index(self._h, fd, size, _kind(kind), os.fsencode(tmpdir),
                                                   os.fsencode(outpath), ctypes.byref(res))
        return _result(res, rc)

    def plan(self, size: int):
        """[(lo, hi, wlo, whi)] per slab: slab k owns [lo, hi) and is held as [wlo, whi)."""
        n = len(self.devices)
        arr = [(ctypes.c_uint64 * n)() for _ in range(4)]
        rc = self._lib.shockidx_multi_plan(self._h, size, *arr)
        if rc != L.OK:
            raise L.ShockIdxError(rc, "shockidx_multi_plan failed")
        return [tuple(int(a[k]) for a in arr) for k in range(n)]

    def build_resident(self, size: int, d_win, d_rows, row_cap, kind="record", fmt=None):
        """Windows already in HBM (d_win[k] on devices[k], per plan()); rows stay on the devices.
        Returns (IndexResult, first_record[], rows_owned[])."""
        n = len(self.devices)
        win = (ctypes.c_void_p * n)(*d_win)
        rws = (ctypes.c_void_p * n)(*d_rows)
        cap = (ctypes.c_uint64 * n)(*row_cap)
        first, owned = (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * n)()
        res = L.Result()
        rc = self._lib.shockidx_multi_build_resident(self._h, size, _kind(kind), _fmt(fmt), win, rws, cap, first,
                                                     owned, ctypes.byref(res))
        return _result(res, rc), [int(x) for x in first], [int(x) for x in owned]
