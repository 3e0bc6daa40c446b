"""Nodes and section lists for the sectioned stream over FASTA and SAM sections under anonymize (the
segmented path of sidx_stream.hip: one wave per section, 16 bytes per lane, 1 KiB per step) -- plain,
deterministic generators shared by the CPU pin (tests/test_stream_formats_ref.py) and the GPU tests
(tests/test_gpu_stream_formats.py, tests/kern_stream.py), so that both see the same bytes.

A node here is (name, intended format, data, [(pos, len)], fail): fail is None when every section passes
in the reference, else (section index, error text).  The CPU pin checks every node against the oracle:
the formats detected, the failing section and its text, and the delivered counts."""
import functools
import random

import numpy as np

import anonref
from anonref import ALN, FA_HEAD, SAM_HEAD

PHASES = (0, 1, 7, 15)  # pos % 16 of a section
STEP = 1024             # bytes a wave walks per step
FA_ERR = b"Invalid fasta entry"
SAM_ERR = b"sam alignment fields less than 11"
TYPE_ERR = b"Invalid file type for filter"
FA_AFTER = b">after\nAC\n"      # follows a FASTA section in the node: "\n>" straddles pos + len
SAM_AFTER = b"\n" + ALN + b"\n"  # follows a SAM section: would complete an unterminated last line
SMALL_FASTQ = anonref.SMALL_FASTQ


# ---- packing --------------------------------------------------------------------------------------------
def pack(items, phases=PHASES, tail=5):
    """[(section, bytes after it)] -> (node, [(pos, len)]): section i at pos % 16 == phases[i % len];
    the byte before every section is '\\n' (a section's first '>' is no boundary whatever precedes it);
    the last section ends at data_len with data_len % 16 == tail."""
    buf, secs = bytearray(b"#" * 15 + b"\n"), []
    for i, (d, after) in enumerate(items):
        ph = phases[i % len(phases)]
        last = i == len(items) - 1
        if last:
            ph = (tail - len(d)) % 16
        pad = (ph - len(buf)) % 16 or 16
        buf += b"#" * (pad - 1) + b"\n"
        secs.append((len(buf), len(d)))
        buf += d + (b"" if last else after)
    assert len(buf) % 16 == tail or not items
    return bytes(buf), secs


def _after(fmt):
    return FA_AFTER if fmt == "fasta" else SAM_AFTER if fmt == "sam" else b"\n"


def sorted_nodes(name, fmt, sections, oracle, passing, text, phases=PHASES):
    """As anonref.det_section_nodes packs its inputs: one node of all the sections that pass, and one
    node per failing section with a passing one before and after it."""
    good = [s for s in sections if oracle.filter_fastq(s, "anonymize")[2] is None]
    bad = [s for s in sections if oracle.filter_fastq(s, "anonymize")[2] is not None]
    af = _after(fmt)
    nodes = []
    if good:
        data, secs = pack([(s, af) for s in good], phases)
        nodes.append((f"{name}-passing", fmt, data, secs, None))
    for k, s in enumerate(bad):
        ph = phases[k % len(phases)]
        data, secs = pack([(passing, af), (s, af), (passing, af)], (0, ph, 7))
        nodes.append((f"{name}-failing-{k}", fmt, data, secs, (1, text)))
    return nodes


# ---- item 1: the runs of a subset ------------------------------------------------------------------------
def fasta_records(k, seed=11):
    rng = random.Random(seed)
    out = []
    for i in range(k):
        lines = [bytes(rng.choices(b"ACGT", k=rng.randint(20, 60))) for _ in range(rng.randint(1, 3))]
        out.append(b">s%d d%d\n" % (i, rng.randrange(1000)) + b"\n".join(lines) + b"\n")
    return out


@functools.lru_cache(maxsize=None)
def fasta_subset(nsecs=3000):
    """-> (node, sections): nsecs back-to-back sections, each the run of 1-3 records (100-600 bytes)."""
    rng = random.Random(12)
    parts, secs, pos = [], [], 0
    recs = iter(fasta_records(3 * nsecs))
    for _ in range(nsecs):
        d = b"".join(next(recs) for _ in range(rng.randint(1, 3)))
        while len(d) < 100:
            d += next(recs)
        secs.append((pos, len(d)))
        parts.append(d)
        pos += len(d)
    assert all(100 <= n <= 600 for _, n in secs)
    return b"".join(parts), secs


@functools.lru_cache(maxsize=None)
def sam_subset(nsecs=3000):
    """-> (node, sections): nsecs sections, each 1-4 alignment lines behind a SAM_HEAD-style first line."""
    rng = random.Random(13)
    parts, secs, pos = [], [], 0
    for i in range(nsecs):
        d = SAM_HEAD + b"".join(anonref._aln(7 * i + j) + b"\n" for j in range(rng.randint(1, 4)))
        secs.append((pos, len(d)))
        parts.append(d)
        pos += len(d)
    return b"".join(parts), secs


# ---- item 2: section edges of the wave walk ------------------------------------------------------------
FA_TAIL = b"\n>z\nT\n"


def _fa(n, events):
    """A FASTA section of n bytes: FA_HEAD, 'A's, the events {offset: byte} and FA_TAIL."""
    a = np.full(n, ord("A"), np.uint8)
    a[:len(FA_HEAD)] = np.frombuffer(FA_HEAD, np.uint8)
    a[n - len(FA_TAIL):] = np.frombuffer(FA_TAIL, np.uint8)
    for p, c in events.items():
        assert len(FA_HEAD) <= p < n - len(FA_TAIL), (p, n)
        a[p] = ord(c)
    return a.tobytes()


def fa_edge_sections(ph):
    """[(name, section)] for a section at pos % 16 == ph: the wave's lane chunks end at section offsets
    16 j - ph and its steps at 1024 j - ph."""
    lane, step = 80 - ph, STEP - ph
    out = []
    for what, e in (("lane", lane), ("step", step), ("step2", 2 * STEP - ph)):
        n = e + 200
        out += [
            (f"nl|gt-{what}", _fa(n, {e - 1: "\n", e: ">", e + 3: "\n"})),
            # the first '>' is a boundary, the second is not
            (f"gt|gt-{what}", _fa(n, {e - 10: "\n", e - 1: ">", e: ">", e + 3: "\n"})),
            (f"gt-nl-gt-{what}", _fa(n, {e - 2: ">", e - 1: "\n", e: ">", e + 3: "\n"})),
            (f"nl-gt-gt-{what}", _fa(n, {e - 1: "\n", e: ">", e + 1: ">", e + 4: "\n", e + 70: ">"})),
        ]
    far = 4 * STEP - ph + 5  # FA_HEAD's '\n' carried over steps 1-3, which hold neither byte
    out += [
        ("nl-carried-3-steps", _fa(far + 300, {far: ">", far + 3: "\n"})),
        ("gt-carried-3-steps", _fa(far + 300, {100: ">", far: ">", far + 3: "\n"})),
        ("zero-boundaries", b">x\nACGT\nAAAA"),
        ("one-boundary", b">x\nAC\n>y\nG\n"),
        ("70-boundaries", b">s\nAC\n" * 71),
    ]
    return out


def sam_edge_sections(ph):
    """[(name, section)]: a line's '\\n' as the last byte of a lane chunk / step and as the first of the
    next, lines over several steps, a last piece without '\\n', a section that delivers nothing."""
    lane, step = 80 - ph, STEP - ph

    def line_to(start, nl_at):  # an alignment line starting at `start` whose '\n' is at offset nl_at
        k = nl_at - start - len(ALN)
        assert k >= 0
        return ALN + b"q" * k + b"\n"

    out = []
    for what, e in (("lane", lane), ("step", step), ("step2", 2 * STEP - ph)):
        for d in (-1, 0):
            first = line_to(len(SAM_HEAD), e + d)
            out.append((f"nl-at-{what}{d:+d}", SAM_HEAD + first + ALN + b"\n\n" + ALN + b" \n"))
    out += [
        ("line-over-4-steps", SAM_HEAD + line_to(len(SAM_HEAD), 4 * STEP + 17 - ph) + ALN + b"\n"),
        ("unterminated-last", SAM_HEAD + ALN + b"\n" + ALN),
        ("unterminated-bad-last", SAM_HEAD + ALN + b"\nr9\t0\t*"),
        ("head-only", SAM_HEAD),
        ("blank-and-comment-lines", SAM_HEAD + b"\n@CO x\n \t\n" + ALN + b"\n"),
    ]
    return out


def edge_nodes(oracle):
    nodes = []
    for ph in PHASES:
        nodes += sorted_nodes(f"fa-edge-{ph}", "fasta", [s for _, s in fa_edge_sections(ph)], oracle, FA_HEAD + b">y\nG\n",
                              FA_ERR, (ph,))
        nodes += sorted_nodes(f"sam-edge-{ph}", "sam", [s for _, s in sam_edge_sections(ph)], oracle, SAM_HEAD + ALN + b"\n",
                              SAM_ERR, (ph,))
    return nodes


# ---- item 4: Read's rules inside small sections ---------------------------------------------------------
def rules_nodes(oracle):
    fa = anonref.fa_gt_runs() + anonref.fa_leading_newlines() + anonref.fa_tile_spanning() + [anonref.fa_trims()[0]]
    sam = [d for d, _ in anonref.sam_field_edges()] + [d for _, d in anonref.sam_eof_cases()] + [anonref.sam_long_lines()]
    return (sorted_nodes("fa-rules", "fasta", fa, oracle, FA_HEAD + b">y\nG\n", FA_ERR)
            + sorted_nodes("sam-rules", "sam", sam, oracle, SAM_HEAD + ALN + b"\n", SAM_ERR))


# ---- item 3: the counter --------------------------------------------------------------------------------
def counter_node():
    """A FASTA section of 120 sequences followed by one of 12 (121 and 13 reads: the last is dropped)."""
    a = b"".join(b">a%d\nACGT\n" % i for i in range(121))
    b = b"".join(b">b%d\nTG\nCA\n" % i for i in range(13))
    return a + b, [(0, len(a)), (len(a), len(b))]


# ---- item 5: the first failure -------------------------------------------------------------------------
GOOD_FA = b">g1\nAC\n>g2\nGT\n>g3\nA\n"
BAD_FA = b">g1\nAC\n>bad\n>g3\nA\n>g4\nT\n"      # the second read has no body
BAD2_FA = b">g1\nAC\n>bad\n>g3\nA\n>bad2\n>g5\nT\n"  # two failing reads in one section
BAD_FQ = b"@r1\nACGT\n+\nIII\n@r2\nAC\n+\nII\n"  # sequence and quality lengths differ
GOOD_SAM = SAM_HEAD + ALN + b"\n" + ALN + b"\n"
BAD_SAM = SAM_HEAD + ALN + b"\nr2\t0\t*\n" + ALN + b"\n"


def _cat(parts):
    secs, pos = [], 0
    for p in parts:
        secs.append((pos, len(p)))
        pos += len(p)
    return b"".join(parts), secs


def first_failure_nodes():
    """(name, fmt, data, secs, fail)"""
    out = []
    d, s = _cat([GOOD_FA, GOOD_FA, BAD_FA, GOOD_FA, BAD_FA, GOOD_FA])
    out.append(("fa-two-sections-fail", "fasta", d, s, (2, FA_ERR)))
    d, s = _cat([GOOD_FA, BAD2_FA, GOOD_FA])
    out.append(("fa-two-in-one-section", "fasta", d, s, (1, FA_ERR)))
    d, s = _cat([GOOD_FA, BAD_FA, SMALL_FASTQ, BAD_FQ])
    out.append(("fa-batch-then-fq-batch", "mixed", d, s, (1, FA_ERR)))
    d, s = _cat([GOOD_SAM, GOOD_SAM, BAD_SAM, BAD_SAM, GOOD_SAM])
    out.append(("sam-two-sections-fail", "sam", d, s, (2, SAM_ERR)))
    d, s = _cat([SMALL_FASTQ, GOOD_SAM, BAD_FQ, BAD_SAM])
    out.append(("fq-fails-before-sam", "mixed", d, s, (2, b"Invalid format: length of sequence and quality lines do not match")))
    return out


# ---- item 6: mixed lists --------------------------------------------------------------------------------
JUNK = b"hello world\n"


def alternating_node(reps=3):
    """FASTQ / FASTA / SAM alternating `reps` times, then junk, then FASTQ -> (data, secs, junk index)."""
    parts = [SMALL_FASTQ, GOOD_FA, GOOD_SAM] * reps + [JUNK, SMALL_FASTQ]
    d, s = _cat(parts)
    return d, s, 3 * reps


def unaligned_batches_node():
    """A FASTQ batch whose output length is odd, then a FASTA batch, then a SAM batch: the second and
    third batch start off a 16-byte boundary of the output (the staged write of each writer)."""
    fq = [b"@r%d\nACGTA\n+\nIIIII\n" % i for i in range(5)]
    fa = [b">s\nAC\n" * 30, GOOD_FA, b">t\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n" * 9]
    sam = [GOOD_SAM, SAM_HEAD + anonref._aln(5) + b"\n", GOOD_SAM]
    return _cat(fq + fa + sam)
