"""GPU: the FASTA boundary scan of anonymize (sidx_filter.hip: k_fa_last, the two max scans, k_fa_bnd,
the sum scan, k_fa_bwrite) launched directly (tests/kern.py, FaBoundaryJob), against
anonref.fasta_boundaries and nothing else.  This is the path a FASTA section takes when its record
index fails but Read carries on; through the public entry points only sections of about one tile reach
it in the suite, so the carries between tiles, the 64-entry slot limit and the byte-wise tail of
masks64 are driven here:

  tcnt    per tile, the reference's boundaries inside the tile
  toff    their exclusive sum
  slot    for every tile of at most sidx_fa_slot() boundaries, the tile-relative positions
  B       whole, and the guard words past it intact (0xAB)

The counts are compared before the writer is launched, so a wrong count fails in Python and never
reaches k_fa_bwrite (which trusts toff)."""
import numpy as np
import pytest

import anonref
import kern

pytestmark = pytest.mark.gpu
TILE = anonref.TILE
_AB64 = np.uint64(0xABABABABABABABAB)


def _check(ctx, buf, what):
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    exp = anonref.fasta_boundaries(buf)
    nt, fslot = (len(buf) + TILE - 1) // TILE, kern.fa_slot()
    tile_of = (exp // np.uint64(TILE)).astype(np.int64)
    exp_cnt = np.bincount(tile_of, minlength=nt).astype(np.uint64)
    exp_off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(exp_cnt, dtype=np.uint64)])
    job = kern.FaBoundaryJob(ctx, buf)
    try:
        tcnt, toff, slot = job.count()
        kern.first_diff(tcnt, exp_cnt, f"{what}: tcnt")
        kern.first_diff(toff, exp_off[:-1], f"{what}: toff")
        for t in np.flatnonzero(exp_cnt <= fslot).tolist():
            mine = exp[int(exp_off[t]):int(exp_off[t + 1])] - np.uint64(t * TILE)
            kern.first_diff(slot[t, :len(mine)], mine.astype(np.uint16), f"{what}: slot of tile {t}")
        K = int(toff[-1] + tcnt[-1])
        assert K == len(exp)
        got = job.write(K)
        kern.first_diff(got[:K], exp, f"{what}: B")
        assert bool((got[K:] == _AB64).all()), f"{what}: wrote past B"
    finally:
        job.free()
    return exp_cnt


def test_slot_constant(gpu_ctx):
    assert kern.fa_slot() == anonref.FSLOT == 64


@pytest.mark.parametrize("n", anonref.BND_SIZES)
def test_fa_boundaries_sizes_gpu(gpu_ctx, n):
    """masks64's byte-wise tail (a + 64 > n), lengths that are no multiple of 16 or 64, a last tile of
    one byte (TILE + 1): k_fa_last and k_fa_bnd skip the words at and past n."""
    buf = anonref.bnd_sized(n)
    assert len(buf) == n
    _check(gpu_ctx, buf, f"n={n}")


def test_fa_boundaries_carries_gpu(gpu_ctx):
    """cin_nl / cin_gt of k_fa_bnd from the max scans over k_fa_last's tile maxima (a '\\n' carried over
    two tiles that hold neither byte; a later '>' that cancels it), word_carry's scan over the 64 words of
    a wave and its LDS step over the four waves of a tile, and bnd_bits' in-word `below` masks: '\\n' | '>'
    and '>' | '>' across a tile edge, a 4096-byte wave edge and a 64-byte word edge."""
    for name, buf in anonref.bnd_carry_cases():
        _check(gpu_ctx, buf, name)


def test_fa_boundaries_slot_limit_gpu(gpu_ctx):
    """Tiles of exactly 0, 1, 63, 64, 65 and 8192 boundaries: k_fa_bnd's `total <= FSLOT` (the slot is
    written or not), k_fa_bwrite's `c_t <= FSLOT` (from the slot, or recomputed with block_excl_add over
    the base from toff), with both kinds alternating in toff."""
    buf = anonref.bnd_slot_limit()
    cnt = _check(gpu_ctx, buf, "slot-limit")
    assert cnt.tolist() == anonref.BND_SLOT_TILES


def test_fa_boundaries_second_scan_block_gpu(gpu_ctx):
    """scan_block + 2 tiles: the max scans and the sum scan run over more than one scan block, with a
    '\\n' carried from tile 2 to the first tile of the second block and overflow tiles on both sides."""
    B = kern.scan_block()
    buf = anonref.bnd_second_scan_block(B)
    assert len(buf) == (B + 2) * TILE
    cnt = _check(gpu_ctx, buf, "second-scan-block")
    assert int(anonref.fasta_boundaries(buf)[-1]) == len(buf) - 1
    assert cnt[1] > kern.fa_slot() and cnt[B] == 1 and cnt[B + 1] > kern.fa_slot() and int(cnt.sum()) == int(cnt[1] + cnt[B] + cnt[B + 1])


@pytest.mark.parametrize("seed", range(8))
def test_fa_boundaries_random_gpu(gpu_ctx, seed):
    buf = anonref.bnd_random(seed)
    assert 4 * TILE < len(buf) <= 9 * TILE
    _check(gpu_ctx, buf, f"random-{seed}")
