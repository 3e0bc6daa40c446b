"""The reference of the download plan: a literal transcription of the section-building loops of
shock-server/controller/node/single.go:372-483 (what is appended to s.R, `size`, the first error and
the part it belongs to), composed from oracle.idx_part / oracle.idx_range -- the C restatements of
Idx.Part / Idx.Range pinned by tests/test_oracle_part.py -- and a transcription of SizePart
(node/file/index/virtual.go:50-80).

This pins the composition rule, not Go itself: no Go toolchain is available to the tests, and the
reference holds no vectors for this branch.  tests/test_plan_ref.py checks it against hand-derived
vectors (tests/golden/plan/kats.json), each citing the Go lines it was read from.
"""
PART, RANGE, CHUNK_RANGE, SIZE = 0, 1, 2, 3
M64 = (1 << 64) - 1
E_RANGE = b"Invalid index record range"
E_BOUNDS = b"Index record out of bounds"


def i64(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def _quo(a, b):
    """Go's int64 `/`: truncated towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def parse_int(s):
    """strconv.ParseInt(s, 10, 64) -> int or None (any error)"""
    if not s:
        return None
    neg = s[0] == "-"
    body = s[1:] if s[0] in "+-" else s
    if not body or any(c not in "0123456789" for c in body):
        return None
    v = int(body)
    if v > (1 << 63) - (0 if neg else 1):
        return None
    return -v if neg else v


def size_part(part, size, chunk):
    """SizePart (virtual.go:50-80) -> (pos, length, err); int64 arithmetic wraps"""
    if "-" in part:
        se = part.split("-")
        start, end = parse_int(se[0]), parse_int(se[1])
        if (start is None or end is None or start <= 0 or i64((start - 1) * chunk) > size or end <= 0
                or i64((end - 1) * chunk) > size):
            return 0, 0, E_RANGE
        pos = i64((start - 1) * chunk)
        full = i64(i64((end - 1) * chunk) - i64((start - 1) * chunk))
        if i64(i64(full + chunk) + pos) > size:
            length = i64(full + i64(size - i64(pos + full)))
        else:
            length = i64(full + chunk)
        return pos, length, None
    p = parse_int(part)
    if p is None or p <= 0 or i64((p - 1) * chunk) > size:
        return 0, 0, E_BOUNDS
    pos = i64((p - 1) * chunk)
    if i64(size - pos) < chunk:
        return pos, i64(size - pos), None
    return pos, chunk, None


def plan_ref(oracle, mode, parts, rows, idx_length, rec_rows=None, rec_length=0, file_size=0, chunk_size=0):
    """-> (sections [[pos, len], ...], size, err bytes|None, err_part).  rows / rec_rows None: that
    index file is missing.  On an error the sections are [] and size 0: nothing is streamed."""
    secs, size = [], 0

    def fail(k, err):
        return [], 0, err, k

    for k, p in enumerate(parts):
        if mode == CHUNK_RANGE:  # single.go:403-425
            chunk_recs, err = oracle.idx_range(rows, p, idx_length)
            if err is not None:
                return fail(k, err)
            for c0, c1 in chunk_recs.tolist():
                start = i64(_quo(c0, 16) + 1)
                stop = i64((start - 1) + _quo(c1, 16))
                recs, err = oracle.idx_range(rec_rows, str(start) + "-" + str(stop), rec_length)
                if err is not None:
                    return fail(k, err)
                for pos, ln in recs.tolist():
                    size = i64(size + ln)
                    secs.append([pos, ln])
        elif mode == RANGE:  # :450-460 (and the full-file forms :390-400, :435-445, :507-516)
            recs, err = oracle.idx_range(rows, p, idx_length)
            if err is not None:
                return fail(k, err)
            for pos, ln in recs.tolist():
                size = i64(size + ln)
                secs.append([pos, ln])
        else:  # :467-474; idx.Part is SizePart for the virtual index (virtual.go:46-48)
            if mode == SIZE:
                pos, ln, err = size_part(p, file_size, chunk_size)
            else:
                pos, ln, err = oracle.idx_part(rows, p, idx_length)
            if err is not None:
                return fail(k, err)
            size = i64(size + ln)
            secs.append([pos, ln])
    return secs, size, None, -1
