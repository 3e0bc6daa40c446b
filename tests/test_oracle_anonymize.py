"""CPU: ?filter=anonymize over FASTA and SAM sections (anonymize.go:28-56 through
multi.Reader): the C oracle against known answers read off fasta.go:40-88 / sam.go:44-81 and
their Format functions, and against a literal Python transcription of those loops on random
sections.  Where Go's fasta Read loops forever (an EOF read without '\\n') both end the stream."""
import random

import numpy as np
import pytest

import anonref
import oracle
import pyref
import streamref


def trim_space(b: bytes) -> bytes:
    """bytes.TrimSpace, Unicode-exact: pyref's transcription of Go's (unicode.IsSpace as a literal list
    of code points, utf8.DecodeRune / DecodeLastRune), which shares no code with the C oracle's."""
    return pyref.trim_space(b)


class Reader:
    def __init__(self, data: bytes):
        self.d, self.p = data, 0

    def read_bytes(self, delim: bytes):
        i = self.d.find(delim, self.p)
        if i < 0:
            out, self.p = self.d[self.p:], len(self.d)
            return out, True
        out, self.p = self.d[self.p:i + 1], i + 1
        return out, False


def fasta_read(r: Reader):
    """fasta.go:40-88; returns ("ok", label, body) | ("eof",) | ("err",)."""
    prev = b""
    while True:
        read, eof = r.read_bytes(b">")
        if prev:
            read = prev + read
        if len(read) == 1:
            if eof:
                return ("eof",)
            continue
        if b"\n" not in read:
            if eof:
                return ("eof",)  # Go: endless loop
            prev = read
            continue
        t = trim_space(read.rstrip(b">"))
        lines = t.split(b"\n")
        label = body = b""
        if len(lines) > 1:
            label, body = lines[0], b"".join(lines[1:])
        if eof:
            return ("eof",)
        return ("ok", label, body) if label and body else ("err",)


def sam_read(r: Reader):
    while True:
        line, eof = r.read_bytes(b"\n")
        if eof:
            return ("eof",)
        if line and line[-1:] == b"\r":
            line = line[:-1]
        line = trim_space(line)
        if not line or line[:1] == b"@":
            continue
        if len(line.split(b"\t")) < 11:
            return ("err",)
        return ("ok", line.split(b"\t")[0], line)


def anonymize(data: bytes, fmt: str):
    r, out, k = Reader(data), [], 0
    while True:
        s = fasta_read(r) if fmt == "fasta" else sam_read(r)
        if s[0] == "eof":
            return b"".join(out), k, None
        if s[0] == "err":
            return b"".join(out), k, (b"Invalid fasta entry" if fmt == "fasta" else b"sam alignment fields less than 11")
        k += 1
        out.append(b">%d\n%s\n" % (k, s[2]) if fmt == "fasta" else s[2] + b"\n")


FASTA_KATS = [
    (b">a\nAC\n>b\nGG\n", b">1\nAC\n", None),
    (b">a\nAC\nGT\n>b x\nG\n>c\nTT", b">1\nACGT\n>2\nG\n", None),
    (b">a\nAC\n>b\n>c\nA\n", b">1\nAC\n", b"Invalid fasta entry"),
    (b">a x>y\nAC\n>b\nGG\n", b">1\nAC\n", None),
    (b">h>\nAC\n>b\nG\n>c\n", b">1\nAC\n>2\nG\n", None),
    (b">a\r\nAC\r\nGT\r\n>b\r\n", b">1\nAC\rGT\n", None),
    (b">>a\nAC\n>b\nC\n", b">1\nAC\n", None),
    (b">a\nAC\n>", b">1\nAC\n", None),
    (b">a\nAC\n>b", b">1\nAC\n", None),
]

SAM_HEAD, ALN = anonref.SAM_HEAD, anonref.ALN
SAM_KATS = [
    (SAM_HEAD + ALN + b"\n" + ALN + b"\n", ALN + b"\n" + ALN + b"\n", None),
    (SAM_HEAD + ALN + b"\n\n @x\n" + ALN, ALN + b"\n", None),
    (SAM_HEAD + ALN + b"\r\n" + b"r2\t0\t*\n" + ALN + b"\n", ALN + b"\n", b"sam alignment fields less than 11"),
    (SAM_HEAD + b"  " + ALN + b" \t\n", ALN + b"\n", None),
]


@pytest.mark.parametrize("data,exp,err", FASTA_KATS + SAM_KATS)
def test_kats(data, exp, err):
    fmt = "fasta" if data[:1] == b">" else "sam"
    assert oracle.detect(data)[0] == fmt
    out, k, e = anonymize(data, fmt)
    assert (out, e) == (exp, err)
    got, gk, ge = oracle.filter_fastq(data, "anonymize")
    assert (got, gk, ge) == (exp, k, err)


def _fasta_corpus(rng):
    parts = []
    for i in range(rng.randint(0, 40)):
        nl = b"\r\n" if rng.random() < 0.2 else b"\n"
        head = b">" * rng.choice([1, 1, 1, 2]) + b"s%d" % i + (b" d>x" if rng.random() < 0.2 else b"")
        if rng.random() < 0.1:
            head += b">"
        body = nl.join(bytes(rng.choice(b"ACGT ") for _ in range(rng.randint(0, 90))) for _ in range(rng.randint(0, 4)))
        parts.append(head + nl + body + (nl if rng.random() < 0.9 else b""))
    return b">x\nA\n" + b"".join(parts)


def _sam_corpus(rng):
    lines = [SAM_HEAD]
    for i in range(rng.randint(0, 40)):
        c = rng.random()
        if c < 0.1:
            lines.append(b"@CO\tx\n")
        elif c < 0.2:
            lines.append(b" \n")
        elif c < 0.25:
            lines.append(b"r%d\t0\t*\n" % i)
        else:
            lines.append(b"r%d\t0\tc\t1\t60\t4M\t*\t0\t0\tACGT\tIIII" % i + (b"\r\n" if c > 0.9 else b"\n"))
    data = b"".join(lines)
    return data if rng.random() < 0.7 else data[: rng.randint(len(SAM_HEAD), len(data))]


def test_random_sections_agree():
    rng = random.Random(12)
    for _ in range(300):
        data = _fasta_corpus(rng)
        exp = anonymize(data, "fasta")
        got = oracle.filter_fastq(data, "anonymize")
        assert got == exp, data
        data = _sam_corpus(rng)
        if oracle.detect(data)[0] != "sam":
            continue
        assert oracle.filter_fastq(data, "anonymize") == anonymize(data, "sam"), data


# ---- the sections and detection inputs of tests/anonref.py: the references the GPU tests rely on, each
# pinned against a second, independent one ------------------------------------------------------------
FASTA_SECTIONS = anonref.fasta_sections()
SAM_SECTIONS = anonref.sam_sections()
DETECT_INPUTS = anonref.detect_inputs()


def _boundaries_slow(d: bytes):
    """fasta_boundaries byte by byte."""
    out, lnl, lgt = [], 0, 0
    for p, c in enumerate(d):
        if c == 0x3E:
            if lnl > lgt:
                out.append(p)
            lgt = p + 1
        elif c == 0x0A:
            lnl = p + 1
    return out


def test_fasta_boundaries_reference():
    rng = random.Random(3)
    for _ in range(400):
        d = bytes(rng.choice(b">>\n\nA\r") for _ in range(rng.randint(0, 80)))
        assert anonref.fasta_boundaries(d).tolist() == _boundaries_slow(d), d
    for name, buf in anonref.bnd_carry_cases()[:8] + [("sized", anonref.bnd_sized(4097)), ("random", anonref.bnd_random(0))]:
        assert anonref.fasta_boundaries(buf).tolist() == _boundaries_slow(buf.tobytes()), name
    per_tile = np.bincount((anonref.fasta_boundaries(anonref.bnd_slot_limit()) // anonref.TILE).astype(np.int64),
                           minlength=len(anonref.BND_SLOT_TILES))
    assert per_tile.tolist() == anonref.BND_SLOT_TILES


def test_trim_space_references_agree():
    """The transcription's TrimSpace (pyref) and the C oracle's on every trim of anonref.TRIMS, alone,
    doubled, at both ends and cut short."""
    assert trim_space(b"AC\xc2\xa0") == b"AC" and trim_space(b"\xe3\x80\x80AC\xe3\x80") == b"AC\xe3\x80"
    for t in anonref.TRIMS:
        for u in anonref.TRIMS:
            for d in (t + b"AC" + u, t + u + b"A\nC" + u + t, t + u, b"A" + t[:-1] + u, t[1:] + b"A" + u[:1]):
                assert trim_space(d) == oracle.trim_space(d), d


@pytest.mark.parametrize("fmt,data", [("fasta", d) for _, d in FASTA_SECTIONS] + [("sam", d) for _, d in SAM_SECTIONS],
                         ids=[f"fasta-{n}" for n, _ in FASTA_SECTIONS] + [f"sam-{n}" for n, _ in SAM_SECTIONS])
def test_generated_sections(fmt, data):
    """Every generated section detects as the format it is meant for, and the oracle's anonymize equals
    the transcription in output, count and error."""
    assert oracle.detect(data)[0] == fmt
    got = oracle.filter_fastq(data, "anonymize")
    assert got == anonymize(data, fmt)
    if fmt == "fasta" and got[2] is None:
        # the reads are the pieces between boundaries: one more than there are boundaries, and the last
        # (to EOF) comes back with io.EOF and is dropped -- so every boundary ends a delivered sequence
        assert len(anonref.fasta_boundaries(data)) + 1 == got[1] + 1


def test_generated_sections_are_what_they_are_for():
    """The properties the GPU cases depend on, asserted on the oracle (no case may quietly stop testing
    its path)."""
    sec = dict(FASTA_SECTIONS)
    n = {k: oracle.filter_fastq(v, "anonymize")[1:] for k, v in sec.items() if not k.startswith(("gt", "tile", "lead"))}
    assert n["many"] == (269_999, None) and n["many"][0] > 262_144
    assert n["natural-fallback"] == (100_000, None)
    assert oracle.record_index(sec["natural-fallback"], "fasta")[1] is not None
    assert n["trims"] == (anonref.fa_trims()[1], None)  # every trim case is delivered: none hides behind an error
    assert n["mid-errors"] == (6, b"Invalid fasta entry")
    assert n["many-two-errors"] == (7, b"Invalid fasta entry")
    assert all((b - 1) % 262_144 == w for b, w in zip(anonref.FA_TWO_ERRORS, (7, 3)))
    for k, v in sec.items():
        if k.startswith("leading-newlines"):
            assert oracle.filter_fastq(v, "anonymize") == (b"", 0, b"Invalid fasta entry")
    for d, exp in zip(anonref.FA_GT_SMALL, [(b">1\nAC\n>2\nGT\n", 2, None), (b">1\nAC\n", 1, b"Invalid fasta entry"),
                                            (b">1\nAC\n>2\nG\n>3\nT\n", 3, None), (b">1\nAC\n", 1, b"Invalid fasta entry"),
                                            (b">1\nAC\n", 1, b"Invalid fasta entry")]):
        assert oracle.filter_fastq(d, "anonymize") == exp, d
    sam = dict(SAM_SECTIONS)
    assert sam["many"].count(b"\n") == 270_001
    out, k, err = oracle.filter_fastq(sam["many"], "anonymize")
    assert err is None and 25_000 < k < 29_000
    out, k, err = oracle.filter_fastq(sam["many-mid-error"], "anonymize")
    assert err == b"sam alignment fields less than 11" and 10_000 < k < 20_000
    assert oracle.filter_fastq(sam["long-lines"], "anonymize")[1:] == (3 * len(anonref.SAM_LINE_LENGTHS), None)
    for (d, fate) in anonref.sam_field_edges():
        k, err = oracle.filter_fastq(d, "anonymize")[1:]
        assert (k, err) == {True: (3, None), None: (2, None), False: (1, b"sam alignment fields less than 11")}[fate], d
    eof = dict(anonref.sam_eof_cases())
    assert oracle.filter_fastq(eof["bad-middle-unterminated-last"], "anonymize")[1:] == (1, b"sam alignment fields less than 11")
    assert oracle.filter_fastq(eof["bad-last-unterminated"], "anonymize")[1:] == (2, None)  # EOF wins
    assert oracle.filter_fastq(eof["ends-in-newline"], "anonymize")[1:] == (2, None)
    assert oracle.filter_fastq(eof["head-only"], "anonymize") == (b"", 0, None)


def test_stream_nodes_reference():
    """The nodes of the sectioned-stream cases: the composition rule over the oracle gives the record
    counts the device's size_only route must report, and the failing section."""
    sam = dict(SAM_SECTIONS)
    node, secs = anonref.stream_node(sam["many"])
    out, count, err, esec = streamref.stream_ref(oracle, "anonymize", node, secs)
    assert (err, esec) == (None, -1) and count == 2 + oracle.filter_fastq(sam["many"], "anonymize")[1] + 100_000 + 2
    node, secs = anonref.stream_node(sam["many-mid-error"])
    out, count, err, esec = streamref.stream_ref(oracle, "anonymize", node, secs)
    assert (err, esec) == (b"sam alignment fields less than 11", 1)
    assert count == 2 + oracle.filter_fastq(sam["many-mid-error"], "anonymize")[1]


def test_detect_inputs_agree():
    """oracle.detect equals pyref.detect_all (the literal regexes) on every detection input, and the
    window edges fall where they are meant to."""
    got = {}
    for name, d in DETECT_INPUTS:
        fmt, mask = oracle.detect(d)
        names = [n for i, n in enumerate(("fasta", "fastq", "sam")) if mask >> i & 1]
        assert names == pyref.detect_all(d), name
        assert fmt == (names[0] if names else None) == pyref.detect_format(d), name
        got[name] = names
    W = anonref.WINDOW
    assert [got[f"fasta-seq-at-{o}"] for o in range(W - 4, W + 1)] == [["fasta"]] * 4 + [[]]
    assert got["fasta-lead-nl-32764"] == ["fasta"] and got["fasta-lead-cr-32765"] == []
    assert [got[f"fastq-final-nl-at-{o}"] for o in range(W - 3, W + 1)] == [["fastq"]] * 3 + [[]]
    assert got["fastq-empty-quality"] == ["fastq"] and got["fastq-no-final-newline"] == []
    assert [got[f"sam-nl-at-{o}"] for o in range(W - 2, W + 1)] == [["sam"]] * 2 + [[]]
    assert got["D1"] == ["fastq", "sam"] and got[f"fastq+sam-final-nl-at-{W}"] == ["sam"]
    # every ballot-step input that ends its run with the regex's next byte matches; the "-after" ones do not
    for name, d in anonref.det_ballot_steps():
        assert bool(got[name]) == (not name.endswith("-after")), name


def test_detect_section_nodes_reference():
    """The nodes for k_detect_sections: every section keeps, inside its node, the result it gives
    alone (the composition rule cuts it out), and each node ends where it is meant to."""
    ok = lambda d: oracle.filter_fastq(d, "anonymize")[2] is None  # noqa: E731
    nodes = anonref.det_section_nodes(ok)
    assert all(len(secs) <= 40 and len(node) % 16 == 5 and secs[-1][0] + secs[-1][1] == len(node) for node, secs in nodes)
    assert {p % 16 for node, secs in nodes for p, _ in secs[:-1]} >= {0, 1, 7, 15}
    none = 0
    for node, secs in nodes:
        out, count, err, esec = streamref.stream_ref(oracle, "anonymize", node, secs)
        if len(secs) > 4:
            assert (err, esec) == (None, -1)
        else:
            assert esec == 1 and err is not None
            none += err == b"Invalid file type for filter"
    assert none >= 4 * 10  # most failing sections fail in the detection itself
