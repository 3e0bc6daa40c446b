"""The composition rule of the sectioned stream (request/streamer.go:78-98): the Streamer builds a new
filter reader for every section (s.Filter(sr), :80-82) and copies each to the client in list order, so
the stream is the per-section filter outputs back to back, ending after the first section whose reader
fails (its bytes before the error are already out; ESection = that section, :92-95).

Each section's own output comes from the oracle's single-section filter over exactly data[pos:pos+len]."""
import json
import os

KATS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream", "kats.json")


def stream_ref(oracle, name, data, sections):
    """-> (bytes delivered, records delivered, error text | None, failing section | -1)"""
    out, count = [], 0
    for i, (pos, ln) in enumerate(sections):
        o, n, err = oracle.filter_fastq(bytes(data[pos:pos + ln]), name)
        out.append(o)
        count += n
        if err is not None:
            return b"".join(out), count, err, i
    return b"".join(out), count, None, -1


def load_kats():
    """[(id, filter, data, [(pos, len)], expected out, failing section, error text | None)]"""
    with open(KATS_PATH) as f:
        raw = json.load(f)
    return [(k["id"], k["filter"], bytes.fromhex(k["data"]), [tuple(s) for s in k["sections"]],
             bytes.fromhex(k["out"]), k["err_section"], k["err"].encode() if k["err"] is not None else None)
            for k in raw]
