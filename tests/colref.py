"""CreateColumnIndex restated line by line in Python (index/column.go:33-130 of the reference
server), plus the closed form the device build computes.  Test support only.

column_index(data, column) walks the Go loop statement by statement and returns
    ("ok", rows)   rows = [(offset, length), ...] as written to the .idx file
    ("err",)       column.go:75-77 returned "Specified column does not exist for all lines in file."
    ("panic",)     slices[column-1] at :79 is out of range (len(slices) == column-1)
closed_form(data, column) is rules 1-6 of the library's definition: it returns ("ok", rows) or
("err",) and maps the panic to the error.
"""
MESSAGE = b"Specified column does not exist for all lines in file."


def read_lines(data: bytes):
    """bufio.Reader.ReadBytes('\\n') until io.EOF: (piece, eof) pairs; the last piece may be empty."""
    pos, n = 0, len(data)
    while True:
        q = data.find(b"\n", pos)
        if q < 0:
            yield data[pos:], True
            return
        yield data[pos:q + 1], False
        pos = q + 1


def column_index(data: bytes, column: int):
    rows = []
    curr = 0
    total_n = 0
    line_count = 0
    prev_str = b""
    for buf, eof in read_lines(data):          # :53-62
        n = len(buf)
        if n <= 1:                             # :64-72
            total_n += n
            line_count += 1
            if eof:
                break
            continue
        slices = buf.split(b"\t")              # :74
        if len(slices) < column - 1:           # :75-77
            return ("err",)
        if column - 1 >= len(slices):          # :79 index out of range
            return ("panic",)
        s = slices[column - 1]
        if prev_str != s and line_count != 0:  # :80-98
            rows.append((curr, total_n))
            curr += total_n
            total_n = 0
            prev_str = s
        if line_count == 0:                    # :99-101
            prev_str = s
        total_n += n                           # :102-103
        line_count += 1
        if eof:                                # :105-107
            break
    if curr != 0:                              # :119-125
        rows.append((curr, total_n))
    return ("ok", rows)


def closed_form(data: bytes, column: int):
    size = len(data)
    cuts = []
    prev = b""
    off = 0
    i = 0
    for buf, _eof in read_lines(data):
        n = len(buf)
        if n > 1:
            t = buf.count(b"\t")
            if t + 1 < column:
                return ("err",)
            key = buf.split(b"\t")[column - 1]
            if i != 0 and key != prev:
                cuts.append(off)
            prev = key
        off += n
        i += 1
    if not cuts:
        return ("ok", [])
    pts = [0] + cuts + [size]
    return ("ok", [(pts[k], pts[k + 1] - pts[k]) for k in range(len(pts) - 1)])


def expected(data: bytes, column: int):
    """What the library must return: ("ok", rows) or ("err",), the panic mapped to the error."""
    r = column_index(data, column)
    return ("err",) if r[0] == "panic" else r
