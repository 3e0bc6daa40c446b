"""References and inputs for the anonymize filter over FASTA and SAM sections and for the format
detection that chooses between them -- plain functions, shared by the CPU pins
(tests/test_oracle_anonymize.py) and the GPU tests (test_gpu_fa_boundaries.py,
test_gpu_anonymize_sections.py, test_gpu_detect_edges.py).  Every generator is deterministic: the
same call gives the same bytes, so the CPU pins and the GPU tests see the same inputs.

fasta_boundaries is the exact boundary set of fasta.go:100-138 in numpy; the generators build the
inputs at which the kernels of sidx_filter.hip / sidx_control.hip change path (16 KiB tiles, 64-byte
words, the 64-entry boundary slot, the 32768-byte detection window)."""
import functools
import random

import numpy as np

TILE = 16384     # SIDX_TILE: bytes per workgroup tile of the boundary scan
WINDOW = 32768   # bytes of a section DetermineFormat reads (multi.go:43-62)
FSLOT = 64       # sidx_fa_slot(): boundaries a tile keeps in its slot (the GPU tests assert the value)
SAM_HEAD = b"@A x\n"  # sam.go:17 needs [@A-Z[][A-Z][ \t]+ at the head ("@HD\t" does not match)
ALN = b"r1\t0\tchr1\t1\t60\t4M\t*\t0\t0\tACGT\tIIII"
FA_HEAD = b">x\nACGT\n"  # makes a section detect as FASTA whatever follows


# ---- the boundary reference -------------------------------------------------------------------------
def _excl_max(v):
    out = np.zeros(len(v), np.int64)
    if len(v) > 1:
        out[1:] = np.maximum.accumulate(v)[:-1]
    return out


def fasta_boundaries(buf) -> np.ndarray:
    """Positions p with buf[p] == '>' whose last '\\n' before p lies after the last '>' before p
    (fasta.go:100-138: the reads end there), as uint64 in ascending order.  Both "last ... before p"
    are exclusive running maxima of position + 1 (0: none); bytes that are neither '\\n' nor '>' do not
    change either maximum, so the maxima run over those two bytes' positions only."""
    a = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
    assert a.dtype == np.uint8 and a.ndim == 1
    ev = np.flatnonzero((a == 10) | (a == 62)).astype(np.int64)
    gt = a[ev] == 62
    last_nl = _excl_max(np.where(gt, 0, ev + 1))
    last_gt = _excl_max(np.where(gt, ev + 1, 0))
    return ev[gt & (last_nl > last_gt)].astype(np.uint64)


def _arr(b) -> np.ndarray:
    return np.frombuffer(bytes(b), np.uint8).copy()


def _fill(n, events):
    """n bytes of 'A' with the given {position: byte}."""
    a = np.full(n, ord("A"), np.uint8)
    for p, c in events.items():
        a[p] = c if isinstance(c, int) else ord(c)
    return a


# ---- part 2: buffers for the boundary scan by direct launch -------------------------------------------
BND_SIZES = [1, 15, 16, 63, 64, 65, 4095, 4096, 4097, TILE - 1, TILE, TILE + 1, 3 * TILE + 17]


def bnd_sized(n: int) -> np.ndarray:
    """n bytes from an alphabet heavy in '>' and '\\n' (the masks64 tail, sizes that are no multiple of
    16 or 64, a last tile of one byte)."""
    rng = np.random.default_rng(4000 + n)
    return rng.choice(np.frombuffer(b">>>\n\n\nAC\r ", np.uint8), n)


def bnd_carry_cases():
    """[(name, buffer)]: carries between tiles (cin_nl / cin_gt of k_fa_bnd), between the waves of a
    tile (4096 bytes each) and between the 64-byte words of a wave (word_carry)."""
    T = TILE
    cases = [
        # '\n' only in tile 0, tiles 1 and 2 hold neither byte, '>' opens tile 3: a boundary
        ("nl-carried-3-tiles", _fill(4 * T, {100: "\n", 3 * T: ">"})),
        # the same with a '>' after the '\n' in tile 0: the '>' of tile 3 is no boundary
        ("gt-carried-3-tiles", _fill(4 * T, {100: "\n", 200: ">", 3 * T: ">"})),
        # the carried '\n' is older than a carried '>' of a later tile
        ("gt-later-tile", _fill(4 * T, {100: "\n", T + 5: ">", 3 * T: ">"})),
        # nothing at all before the first '>' (both carries 0: 0 > 0 is false)
        ("gt-first-no-nl", _fill(2 * T + 3, {T: ">", T + 1: "\n", 2 * T + 2: ">"})),
    ]
    for name, edge in (("tile", 2 * T), ("word", T + 64), ("wave", T + 4096), ("last-word", 2 * T - 64)):
        cases += [
            (f"nl|gt-at-{name}-edge", _fill(3 * T, {edge - 1: "\n", edge: ">"})),
            # the first '>' is a boundary (a '\n' before it), the second is not
            (f"gt|gt-at-{name}-edge", _fill(3 * T, {edge - 10: "\n", edge - 1: ">", edge: ">"})),
            (f"gt|nl|gt-at-{name}-edge", _fill(3 * T, {7: "\n", edge - 2: ">", edge - 1: "\n", edge: ">"})),
            (f"nl|gt-then-gt-{name}-edge", _fill(3 * T, {edge - 1: "\n", edge: ">", edge + 1: ">", edge + 70: ">"})),
        ]
    return cases


BND_SLOT_TILES = [64, 65, 0, 8192, 1, 65, 63, 8192, 64, 0, 65, 1]  # boundaries per tile, slot / overflow alternating


def bnd_slot_limit() -> np.ndarray:
    """One tile per entry of BND_SLOT_TILES holding exactly that many boundaries ("\\n>" repeated, then
    filler; 8192 pairs fill the tile: the densest possible), so tiles served from their slot and tiles
    k_fa_bwrite recomputes alternate and toff mixes both kinds."""
    tiles = []
    for k in BND_SLOT_TILES:
        t = b"\n>" * k
        tiles.append(t + b"A" * (TILE - len(t)))
    return _arr(b"".join(tiles))


def bnd_second_scan_block(scan_block: int) -> np.ndarray:
    """scan_block + 2 tiles of filler with a few '\\n' / '>' at tile edges, carries that cross the edge
    between the first and the second scan block, and overflow tiles on both sides of it (the sum scan's
    carry)."""
    T, nt = TILE, scan_block + 2
    a = np.full(nt * T, ord("A"), np.uint8)
    dense = np.frombuffer(b"\n>" * 70, np.uint8)
    a[T:T + len(dense)] = dense                                   # tile 1: 70 boundaries (no slot), ends in '>'
    a[3 * T - 1] = ord("\n")                                      # last byte of tile 2
    a[scan_block * T] = ord(">")                                  # first tile of block 1: a boundary by the '\n'
    #                                                               carried over every tile between and the block edge
    a[(scan_block + 1) * T] = ord(">")                            # no boundary: the carried '>' is later
    a[(scan_block + 1) * T + 5] = ord("\n")
    a[(scan_block + 1) * T + 100:(scan_block + 1) * T + 100 + len(dense)] = dense
    a[-2], a[-1] = ord("\n"), ord(">")                             # the last byte is a boundary
    return a


def bnd_random(seed: int) -> np.ndarray:
    """5-9 tiles (plus an odd tail) from the alphabet > \\n \\r A C space with '>' and '\\n' at 5-30 % each."""
    rng = np.random.default_rng(7000 + seed)
    n = int(rng.integers(5, 10)) * TILE - int(rng.integers(0, TILE))
    pg, pn = rng.uniform(0.05, 0.30, 2)
    rest = (1.0 - pg - pn) / 4
    return rng.choice(np.frombuffer(b">\n\rAC ", np.uint8), n, p=[pg, pn, rest, rest, rest, rest])


# ---- part 3: FASTA sections ---------------------------------------------------------------------------
def fa_many(k: int = 270_000, bad=()) -> bytes:
    """k sequences ">s%d\\nACGT\\n": more than 262144, the grid stride of k_fa_anon_spans / _write.
    bad: those sequences (counted from 1) are a header with no body."""
    return b"".join(b">s%d\n" % i if i + 1 in bad else b">s%d\nACGT\n" % i for i in range(k))


# wave_grid caps at 65536 blocks x 4 waves: sequence index k runs in wave k % 262144, so the later of
# these two failing sequences (index 262147: wave 3) runs in a lower-numbered wave than the earlier
# (index 7: wave 7)
FA_TWO_ERRORS = (8, 262_148)


def fa_natural_fallback(k: int = 100_001) -> bytes:
    """Headers ending in '>': the record index fails at the first, Read carries on (all but the last,
    which ends at EOF, are delivered)."""
    return b"".join(b">s%d>\nACGT\n" % i for i in range(k))


ASCII_TRIMS = [b"\t", b" ", b"\v", b"\f", b"\r"]
UNI_TRIMS = [0x85, 0xA0, 0x1680, 0x2003, 0x2028, 0x3000]  # unicode.IsSpace beyond ASCII (a selection)
NEAR_MISSES = [b"\xc2\xa1", b"\xe2\x80\x8b", b"\xc2", b"\xe3\x80"]  # kept: no space, or no whole rune
TRIMS = ASCII_TRIMS + [chr(u).encode("utf-8") for u in UNI_TRIMS] + NEAR_MISSES


def fa_trims():
    """-> (section, sequences delivered).  Every entry of TRIMS at the end of a body and at the start
    of a label line, at every sequence length 4..40 that can hold it, each next to a plain sequence
    of the same length class (k_fa_anon_spans: the fast path needs e0 >= s + 4, ASCII non-space bytes
    at both ends; everything else goes through trim_space in lane 0)."""
    parts = [FA_HEAD]
    for t in TRIMS:
        for L in range(4, 41):
            made = []
            if L - 4 - len(t) >= 1:
                made.append(b">a\n" + (b"ACGT" * 10)[:L - 4 - len(t)] + t + b"\n")
            elif L - 3 - len(t) >= 1:  # no room for the '\n': the next '>' follows the trim bytes
                made.append(b">a\n" + (b"ACGT" * 10)[:L - 3 - len(t)] + t)
            if L - 4 - len(t) >= 1:
                made.append(b">" + t + b"b\n" + (b"TGCA" * 10)[:L - 4 - len(t)] + b"\n")
            for m in made:
                assert len(m) == L
                parts += [m, b">p\n" + (b"ACGT" * 10)[:max(L - 4, 1)] + b"\n"]
    parts.append(b">end\nA\n")
    return b"".join(parts), len(parts) - 1  # the last sequence ends at EOF


FA_GT_SMALL = [  # the issue's five sections (results checked against the CPU oracle)
    b">a>\nAC\n>b\nGT\n>c\nA\n",
    b">x\nAC\n>>\n>y\nG\n>z\nT\n",
    b">x\nAC\n>y>\nG\n>z\nT\n>w\nA\n",
    b">x\nAC>\n>y\nG\n>z\nT\n",
    b">x\nAC\n>\n>y\nG\n>z\nT\n",
]
_GT_OK = [b">>a\nAC\n", b">a x>y\nACG\n", b">c\nT\n", b">d>\nAC\nGT\n", b">>>f>>\nA\n", b">h>>i\nG>T\nA\n", b">j\nAC\n\n"]
# Read's error: what is left of the read after TrimRight(">") and TrimSpace holds no '\n'
_GT_ERR = [b">a\nAC>>>\n", b">b\nGGT>\n", b">\n", b">>\n", b">e\nA>\nC\n", b">g\n>AC\n", b">h>>i\nG>T\n"]


def fa_gt_runs():
    """[section]: '>' runs in headers, inside and at the end of bodies and as lone pieces -- the five
    small sections, every piece alone between plain sequences, seeded mixes of the pieces Read accepts,
    and the same mixes with one failing piece two thirds in."""
    out = list(FA_GT_SMALL)
    out += [FA_HEAD + p + b">y\nG\n>z\nT\n" for p in _GT_OK + _GT_ERR]
    rng = random.Random(91)
    for i in range(6):
        mix = [rng.choice(_GT_OK) for _ in range(300)]
        if i % 2:
            mix[200] = _GT_ERR[i // 2 * 2 + rng.randrange(2)]
        out.append(FA_HEAD + b"".join(mix) + b">z\nT\n")
    return out


def fa_leading_newlines():
    """Sections that detect as FASTA (the regex skips [\\n\\r]*) but whose first read is invalid."""
    body = b">a\nACGT\n>b\nGG\n>c\nT\n"
    return [lead + body for lead in (b"\n", b"\r\n", b"\n\n\r")]


def fa_mid_errors(k: int = 50_000, bad=(49_998, 7)) -> bytes:
    """k sequences with seeded body lengths; the bad-th ones (counted from 1) are a header with no
    body.  Read fails at the earlier one: the sequences before it are delivered."""
    rng = random.Random(5)
    parts = []
    for i in range(1, k + 1):
        if i in bad:
            parts.append(b">h%d\n" % i)
        else:
            parts.append(b">h%d\n" % i + bytes(rng.choices(b"ACGT", k=rng.randint(1, 90))) + b"\n")
    return b"".join(parts)


def fa_tile_spanning():
    """[section]: a sequence whose '>' sits 1-3 bytes before a tile edge, with a body of 0, 1, TILE and
    2 TILE + 5 bytes in CRLF lines (under anonymize the '\\r's stay in the body); a body of 0 bytes is
    Read's error, so every combination is its own section."""
    out = []
    for d in (1, 2, 3):
        for blen in (0, 1, TILE, 2 * TILE + 5):
            head = b">x\r\nACGT\r\n>p\r\n"
            pad = TILE - d - len(head) - 2
            pre = head + b"C" * pad + b"\r\n"
            assert len(pre) == TILE - d
            seq = bytes(b"ACGT"[i % 4] for i in range(blen))
            width = 1000 if blen == TILE else 4093
            lines = b"".join(seq[j:j + width] + b"\r\n" for j in range(0, blen, width))
            out.append(pre + b">t\r\n" + lines + b">z\r\nAC\r\n>e\r\nA\r\n")
    return out


# ---- part 3: SAM sections -----------------------------------------------------------------------------
def _aln(i: int) -> bytes:
    return b"r%d\t0\tchr1\t%d\t60\t4M\t*\t0\t0\tACGT\tIIII" % (i, i % 1000 + 1)


def sam_many(k: int = 270_001, bad_at: int | None = None) -> bytes:
    """k lines after SAM_HEAD: about 55 % "\\n", 30 % "@C\\n", 5 % " \\t\\n", 10 % alignments (more than
    262144 lines: the grid stride of both SAM kernels, most waves deliver nothing).  bad_at: that line
    is an alignment of three fields (Read's error in the middle)."""
    rng = random.Random(2701)
    lines = [SAM_HEAD]
    for i in range(k - 1):
        c = rng.random()
        if i == bad_at:
            lines.append(b"r%d\t0\t*\n" % i)
        elif c < 0.55:
            lines.append(b"\n")
        elif c < 0.85:
            lines.append(b"@C\n")
        elif c < 0.90:
            lines.append(b" \t\n")
        else:
            lines.append(_aln(i) + b"\n")
    return b"".join(lines)


NBSP = b"\xc2\xa0"  # U+00A0
SAM_FIELD_EDGES = [  # (the line, delivered?)  -- tabs are counted in the trimmed line
    (ALN, True),                                        # exactly 10 tabs
    (ALN.rsplit(b"\t", 1)[0], False),                   # 9 tabs
    (b"\t" + ALN.rsplit(b"\t", 1)[0], False),           # 10 tabs, one leading: 9 after the trim
    (ALN.rsplit(b"\t", 1)[0] + b"\t", False),           # 10 tabs, one trailing
    (b" \t " + ALN + b"\t \t", True),                   # 11 fields inside leading / trailing tabs and spaces
    (NBSP + b"\t" + ALN + b"\t" + NBSP, True),          # the same with U+00A0
    (b" @x", None),                                     # skipped: the trimmed line starts with '@'
    (NBSP + NBSP, None),                                # blank after the trim
    (b"\t\t\t\t\t\t\t\t\t\t", None),                     # ten tabs and nothing else: blank
]


def sam_field_edges():
    """[(section, the edge line's fate)]: one section per entry of SAM_FIELD_EDGES (an error ends the
    stream), the line between two good alignments."""
    return [(SAM_HEAD + _aln(1) + b"\n" + ln + b"\n" + _aln(2) + b"\n", fate) for ln, fate in SAM_FIELD_EDGES]


SAM_LINE_LENGTHS = [63, 64, 65, 4096, TILE + 3, 100_000]


def sam_long_lines() -> bytes:
    """Valid 11-field lines whose trimmed text is 63, 64, 65, 4096, TILE + 3 and 100000 bytes long (the
    64-byte wave steps of both SAM kernels, lines that span tiles of the line index), once bare and
    once inside the trim bytes of SAM_FIELD_EDGES, with CRLF endings."""
    lines = [SAM_HEAD]
    for L in SAM_LINE_LENGTHS:
        core = ALN + b"q" * (L - len(ALN))
        assert len(core) == L and core.count(b"\t") == 10
        lines += [core + b"\r\n", b" \t" + NBSP + core + NBSP + b"\t \r\n"]
        whole = core[:L - 2] + b"\r\n"  # the whole line, CRLF included, is L bytes
        lines.append(whole)
    return b"".join(lines)


def sam_eof_cases():
    """[(name, section)]: io.EOF against Read's error."""
    bad = b"r9\t0\t*"
    return [
        ("bad-middle-unterminated-last", SAM_HEAD + _aln(1) + b"\n" + bad + b"\n" + _aln(2) + b"\n" + _aln(3)),
        ("bad-last-unterminated", SAM_HEAD + _aln(1) + b"\n" + _aln(2) + b"\n" + bad),  # EOF wins: no error
        ("ends-in-newline", SAM_HEAD + _aln(1) + b"\n" + _aln(2) + b"\n"),
        ("bad-last-terminated", SAM_HEAD + _aln(1) + b"\n" + bad + b"\n"),
        ("head-only", SAM_HEAD),
    ]


SMALL_FASTQ = b"@r1 x\nACGT\n+\nIIII\n@r2\nAC\n+r2\nII\n"


def stream_node(sam: bytes):
    """-> (node, sections): [small FASTQ, the SAM section, the natural-fallback FASTA section, small
    FASTQ] back to back in one node (the sectioned stream sizes its output first: size_only)."""
    parts = [SMALL_FASTQ, sam, fa_natural_fallback(), SMALL_FASTQ]
    secs, pos = [], 0
    for p in parts:
        secs.append((pos, len(p)))
        pos += len(p)
    return b"".join(parts), secs


@functools.lru_cache(maxsize=None)
def fasta_sections():
    """[(name, section)]: every FASTA section of part 3 (built once per process)."""
    out = [("many", fa_many()), ("natural-fallback", fa_natural_fallback()), ("trims", fa_trims()[0]),
           ("mid-errors", fa_mid_errors()), ("many-two-errors", fa_many(bad=FA_TWO_ERRORS))]
    out += [(f"gt-runs-{i}", d) for i, d in enumerate(fa_gt_runs())]
    out += [(f"leading-newlines-{i}", d) for i, d in enumerate(fa_leading_newlines())]
    out += [(f"tile-spanning-{i}", d) for i, d in enumerate(fa_tile_spanning())]
    return out


SAM_BAD_AT = 135_000  # sam_many's line that fails in the "mid-error" section


@functools.lru_cache(maxsize=None)
def sam_sections():
    """[(name, section)]: every SAM section of part 3."""
    out = [("many", sam_many()), ("many-mid-error", sam_many(bad_at=SAM_BAD_AT)), ("long-lines", sam_long_lines())]
    out += [(f"field-edge-{i}", d) for i, (d, _) in enumerate(sam_field_edges())]
    out += [(f"eof-{n}", d) for n, d in sam_eof_cases()]
    return out


# ---- part 4: detection at its window and lane edges ---------------------------------------------------
def det_window_fasta():
    """[(name, input)]: the first sequence byte at offsets 32764..32768 (the last lies outside the
    window: no match), and leading newlines up to the window's end."""
    out = []
    for off in range(WINDOW - 4, WINDOW + 1):
        d = b">" + b"h" * (off - 2) + b"\n" + b"A\n>b\nA\n"
        assert d[off:off + 1] == b"A"
        out.append((f"fasta-seq-at-{off}", d))
    out.append(("fasta-lead-nl-32764", b"\n" * (WINDOW - 4) + b">a\nA\n"))
    out.append(("fasta-lead-cr-32765", b"\r" * (WINDOW - 3) + b">a\nA\n"))
    out.append(("fasta-gt-at-32767", b"\n" * (WINDOW - 1) + b">a\nA\n"))
    out.append(("fasta-header-nl-at-32767", b">" + b"h" * (WINDOW - 2) + b"\nA\n"))
    return out


def det_window_fastq():
    out = []
    for off in range(WINDOW - 3, WINDOW + 1):
        tail = b"\nAC\n+\nII"
        d = b"@" + b"r" * (off - 1 - len(tail)) + tail + b"\n@s\nA\n+\nI\n"
        assert d[off:off + 1] == b"\n" and d[off - 1:off] == b"I"
        out.append((f"fastq-final-nl-at-{off}", d))
    for off in range(WINDOW - 2, WINDOW + 1):  # an empty quality line: the second '\n' ends the match
        tail = b"\nAC\n+\n"
        d = b"@" + b"r" * (off - 1 - len(tail)) + tail + b"\nII\n"
        assert d[off - 1:off + 1] == b"\n\n"
        out.append((f"fastq-empty-quality-2nd-nl-at-{off}", d))
    out += [
        ("fastq-empty-quality", b"@r\nAC\n+\n\n"),               # k >= 2
        ("fastq-one-nl-then-quality", b"@r\nAC\n+\nII\n"),        # k == 1
        ("fastq-one-nl-then-space", b"@r\nAC\n+\n II\n"),         # k == 1, \S* stops at the space
        ("fastq-no-final-newline", b"@r\nAC\n+\nII"),             # \S* takes the padding: no match
        ("fastq-plus-at-eof", b"@r\nAC\n+"),
    ]
    return out


def det_window_sam():
    out = []
    for off in range(WINDOW - 2, WINDOW + 1):
        d = b"@A " + b"x" * (off - 3) + b"\n" + ALN + b"\n"
        assert d[off:off + 1] == b"\n"
        out.append((f"sam-nl-at-{off}", d))
    out.append(("sam-only-blank-run-to-window-end", b"@A" + b" " * (WINDOW - 2) + b"x\n"))
    return out


RUN_LENGTHS = [63, 64, 65, 127, 128, 129]


def _cyc(alphabet: bytes, n: int) -> bytes:
    return (alphabet * (n // len(alphabet) + 1))[:n]


def _fastq_doc(lead=0, idrun=3, nl1=1, seq=4, nl2=1, plus=0, nl3=1, qual=4, good=True) -> bytes:
    """A FASTQ head with every class run of fastq.go:22 at a chosen length: leading newlines, the ID
    and description ([\\S\\t ]*), the sequence, the plus line, the quality, and the newline runs."""
    return (_cyc(b"\n\r", lead) + b"@r" + _cyc(b"id \t", idrun) + _cyc(b"\n\r", nl1) + _cyc(b"ACgt-", seq)
            + _cyc(b"\r\n", nl2) + b"+" + _cyc(b"p \t", plus) + _cyc(b"\n\r", nl3) + _cyc(b"I#5", qual)
            + (b"\n" if good else b" \n") + b"@s\nA\n+\nI\n")


_FQ_RUNS = ("lead", "idrun", "nl1", "seq", "nl2", "plus", "nl3", "qual")


def _fq_run_start(kw, run):
    """The offset at which det_skip starts on that run."""
    d = dict(lead=0, idrun=3, nl1=1, seq=4, nl2=1, plus=0, nl3=1, qual=4)
    d.update(kw)
    at = {"lead": 0, "idrun": d["lead"] + 2}
    at["nl1"] = at["idrun"] + d["idrun"]
    at["seq"] = at["nl1"] + d["nl1"]
    at["nl2"] = at["seq"] + d["seq"]
    at["plus"] = at["nl2"] + d["nl2"] + 1
    at["nl3"] = at["plus"] + d["plus"]
    at["qual"] = at["nl3"] + d["nl3"]
    return at[run]


def det_ballot_steps():
    """[(name, input)]: every class run of the three regexes at lengths 63..129, starting at offset 0
    and 1 modulo 64 (det_skip's 64-byte ballot steps), each once matching and -- where the byte after
    the run decides -- once with a byte that ends the match."""
    out = []
    for run in _FQ_RUNS:
        for L in RUN_LENGTHS:
            for ph in (0, 1):
                kw = {run: L}
                if run == "lead":
                    if ph:
                        continue  # the leading run starts at offset 0
                else:
                    kw["lead"] = (ph - _fq_run_start(kw, run)) % 64
                    assert _fq_run_start(kw, run) % 64 == ph
                out.append((f"fastq-{run}-{L}-at-{ph}", _fastq_doc(**kw)))
                if run == "qual":
                    out.append((f"fastq-{run}-{L}-at-{ph}-space-after", _fastq_doc(good=False, **kw)))
    for L in RUN_LENGTHS:
        for ph in (0, 1):
            lead = _cyc(b"\r\n", (ph - 2) % 64)  # the header run starts after ">h"
            out.append((f"fasta-header-{L}-at-{ph}", lead + b">h" + _cyc(b"d \t", L) + b"\nACGT\n"))
            out.append((f"fasta-header-{L}-at-{ph}-ff-after", lead + b">h" + _cyc(b"d \t", L) + b"\f\nACGT\n"))
            lead = _cyc(b"\r\n", (ph - 3) % 64)  # ">hd" then the newline run
            out.append((f"fasta-nl-{L}-at-{ph}", lead + b">hd" + _cyc(b"\n\r", L) + b"ACGT\n"))
            out.append((f"fasta-nl-{L}-at-{ph}-digit-after", lead + b">hd" + _cyc(b"\n\r", L) + b"1ACGT\n"))
            lead = _cyc(b"\r\n", (ph - 3) % 64)  # "@A " then the [\S \t]+ run
            out.append((f"sam-text-{L}-at-{ph}", lead + b"@A " + _cyc(b"x \t", L) + b"\n" + ALN + b"\n"))
            out.append((f"sam-text-{L}-at-{ph}-ff-after", lead + b"@A " + _cyc(b"x \t", L) + b"\f\n" + ALN + b"\n"))
        out.append((f"fasta-lead-{L}", _cyc(b"\n\r", L) + b">h\nACGT\n"))
        out.append((f"sam-lead-{L}", _cyc(b"\n\r", L) + b"@A x\n" + ALN + b"\n"))
    return out


def det_two_formats():
    """[(name, input)]: inputs more than one regex matches (the format chosen: FASTA, then FASTQ, then
    SAM).  Every regex is anchored and FASTA's first byte after the newlines is '>', which neither
    FASTQ ('@') nor SAM ([@[A-Z]) accepts: FASTQ + SAM is the only pair that exists."""
    d1 = b"@A desc\nACGT\n+\nIIII\n"
    out = [("D1", d1), ("D1-lead-nl", b"\n\r\n" + d1)]
    # both end inside the window / only SAM does (FASTQ's final newline falls outside)
    for off in (WINDOW - 1, WINDOW):
        tail = b"\nAC\n+\nII"
        d = b"@A " + b"r" * (off - 3 - len(tail)) + tail + b"\n"
        assert d[off:off + 1] == b"\n"
        out.append((f"fastq+sam-final-nl-at-{off}", d))
    return out


def detect_inputs():
    return det_window_fasta() + det_window_fastq() + det_window_sam() + det_ballot_steps() + det_two_formats()


def det_section_nodes(ok):
    """[(node, sections)], at most 40 sections each, for the sectioned stream under anonymize: the
    window-edge FASTA and FASTQ inputs as sections at pos % 16 in {0, 1, 7, 15} (k_detect_sections
    stages from 16-byte aligned loads), sections of 1, 15, 16, 17 and 32767 bytes, short sections
    followed in the node by the bytes that would complete their match, and a last section ending at a
    data_len that is no multiple of 16.  The stream ends at the first section that fails, so ok(section)
    (the reference: no error) sorts them: per phase one node of all the sections that pass, and one node
    per failing section with a passing one before and after it."""
    edge = [d for _, d in det_window_fasta() + det_window_fastq()]
    short = [b">", b">ab\nACGT\n>b\nAC\n", b">abc\nACGT\n>b\nAC\n", b"@r\nAC\n+\nII\n@s\nA\n+",
             (b">a\n" + b"ACGT" * 8192)[:WINDOW - 1]]
    assert [len(d) for d in short] == [1, 15, 16, 17, WINDOW - 1]
    # cut short: what completes the match follows in the node, outside the section
    cut = [(b">abc\n", b"ACGT\n"), (b"@r\nAC\n+\nII", b"\n@s\nA\n+\nI\n"), (b"@r\nAC\n+", b"\n\n"), (b"@A x", b"\n"),
           (b">", b"a\nA\n"), (b"@r\nAC\n+\n", b"\n")]
    items = [(d, b"") for d in edge + short] + cut
    good = [it for it in items if ok(it[0])]
    bad = [it for it in items if not ok(it[0])]
    assert len(good) >= 8 and len(bad) >= 8 and len(good) <= 39
    passing = (b"@r\nAC\n+\nII\n", b"")

    def node(its, ph):
        buf, secs = bytearray(b"#" * 16), []
        for d, after in its:
            buf += b"#" * ((ph - len(buf)) % 16)
            secs.append((len(buf), len(d)))
            buf += d + after
        last = passing[0]  # ends at data_len, data_len % 16 == 5
        buf += b"#" * ((5 - len(buf) - len(last)) % 16)
        secs.append((len(buf), len(last)))
        buf += last
        assert len(buf) % 16 == 5 and len(secs) <= 40
        return bytes(buf), secs

    nodes = []
    for ph in (0, 1, 7, 15):
        nodes.append(node(good, ph))
        nodes += [node([passing, it, passing], ph) for it in bad]
    return nodes
