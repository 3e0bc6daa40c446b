// slabwalk_test.cpp -- CPU test of the slab walk's pure pieces (shock_amd/csrc/sidx_slabwalk.hpp):
// the slab layout, the ring's slab size, the meaning of a slab's device result, the row cursor
// and the end-of-table invariant.  Stand-alone: it includes that header only, links nothing of
// the library and makes no HIP call.  Built with the host sanitizers by
// `make -C shock_amd/csrc slabwalk_test`; exit 0 = every check held.
#include <stdio.h>

#include <vector>

#include "sidx_slabwalk.hpp"

using namespace sidx;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                \
    }                                                            \
  } while (0)

static constexpr u64 MIB = 1ull << 20, GIB = 1ull << 30;
static u64 min64(u64 a, u64 b) { return a < b ? a : b; }

static void test_layout() {
  for (u64 S : {64 * MIB, GIB})
    for (bool ring : {false, true})
      for (u64 n : {2 * S, 2 * S + 1, 3 * S - 1, S + PIPE_HALO - 1, S + PIPE_HALO, S + PIPE_HALO + 1}) {
        const SlabLayout lay{n, S, ring};
        const u64 K = lay.count();
        CHECK(K >= 1);
        u64 next = 0;  // the owned ranges tile [0, n) exactly
        for (u64 k = 0; k < K; ++k) {
          CHECK(lay.lo(k) == next);
          CHECK(lay.len(k) > 0 && lay.len(k) <= S);
          next = lay.lo(k) + lay.len(k);
          CHECK(lay.end(k) == min64(lay.len(k) + PIPE_HALO, n - lay.lo(k)));
          CHECK(lay.front(k) == (ring ? min64(lay.lo(k), RING_FRONT) : lay.lo(k)));
          // eof: the last slab, and an earlier one only when the rest fits its halo
          const bool rest_in_halo = n - lay.lo(k) <= lay.len(k) + PIPE_HALO;
          CHECK(lay.eof(k) == (lay.lo(k) + lay.end(k) == n));
          CHECK(lay.eof(k) == (k + 1 == K || rest_in_halo));
          CHECK(lay.last(k) == (k + 1 == K));
          if (k + 1 == K) CHECK(lay.eof(k));
        }
        CHECK(next == n);
      }
  // a rest shorter than the halo: the slab before the last one already reads to the file's end
  const SlabLayout lay{GIB + PIPE_HALO - 1, GIB, true};
  CHECK(lay.count() == 2 && lay.eof(0) && !lay.last(0) && lay.eof(1) && lay.last(1));
  CHECK((!SlabLayout{GIB + PIPE_HALO + 1, GIB, true}.eof(0)));
}

static void test_ring_slab_bytes() {
  CHECK(ring_slab_bytes(300 * MIB) == 64 * MIB);
  CHECK(ring_slab_bytes(8 * GIB) == GIB);
  const u64 fixed = 2 * (64 * 1024 + 4 * MIB + 64) + 96 * MIB;
  CHECK(RING_FIXED == fixed);
  const u64 two = ring_slab_bytes(2 * GIB);
  CHECK(two % (16 * MIB) == 0);
  CHECK(two == ((2 * GIB - fixed) * 10 / 27) / (16 * MIB) * (16 * MIB));
  CHECK(ring_slab_bytes(0) == 0 && ring_slab_bytes(fixed) == 0);
  // the smallest budget whose share reaches 64 MiB: S = (b - fixed) * 10 / 27 >= 64 MiB
  const u64 first = fixed + (64 * MIB * 27 + 9) / 10;
  CHECK(ring_slab_bytes(first) == 64 * MIB);
  CHECK(ring_slab_bytes(first - 1) == 0);  // the largest budget that yields 0 is adjacent to it
  // found by search as well: monotone, so bisect between a budget that fails and one that works
  u64 lo = fixed, hi = 300 * MIB;
  while (hi - lo > 1) {
    const u64 mid = lo + (hi - lo) / 2;
    (ring_slab_bytes(mid) ? hi : lo) = mid;
  }
  CHECK(ring_slab_bytes(lo) == 0 && ring_slab_bytes(hi) == 64 * MIB && hi == first);
  CHECK(hi - lo <= 16 * MIB);
  for (u64 b = 200 * MIB; b < 4 * GIB; b += 37 * MIB) {  // never more than the formula, never above 1 GiB
    const u64 S = ring_slab_bytes(b);
    CHECK(S <= GIB && S % (16 * MIB) == 0 && (S == 0 || S >= 64 * MIB));
    CHECK(S == 0 || 2 * (RING_FRONT + S + PIPE_HALO + 64) + S * 7 / 10 + 96 * MIB <= b);
  }
}

// the rules of sidx_pipeline.cpp's header comment, restated independently
static SlabOutcome expect_outcome(int rc, u32 flags, u32 code, u64 count, u64 row_base, bool last, bool ring) {
  const bool success = code == ST_OK || (last && (code == ST_END || code == ST_ABSENT));
  if (rc == 0 && flags == 0 && count >= row_base && success) return SlabOutcome::Clean;
  if (!ring || rc != 0 || count < row_base) return SlabOutcome::FallBack;
  if (flags == 0) {
    switch (code) {
      case ST_FQ_TRUNC: return last ? SlabOutcome::GoError : SlabOutcome::FallBack;
      case ST_FQ_EMPTYLINES: case ST_FQ_NOAT: case ST_FQ_NOID: case ST_FQ_EMPTYSEQ: case ST_FQ_NOPLUS:
      case ST_FQ_IDMISMATCH: case ST_FQ_LENMISMATCH: case ST_FA_INVALID:
        return SlabOutcome::GoError;
      case ST_END: return last ? SlabOutcome::FallBack /* (clean above) */ : SlabOutcome::Partial;
      default: return SlabOutcome::FallBack;
    }
  }
  if (flags == 4 && code == ST_NEEDMORE && !last) return SlabOutcome::Partial;
  return SlabOutcome::FallBack;
}

static void test_classify() {
  const int EFORMAT = 1;  // SHOCKIDX_EFORMAT
  const u32 codes[] = {ST_OK, ST_END, ST_ABSENT, ST_FQ_TRUNC, ST_FQ_NOPLUS, ST_FA_INVALID, ST_NEEDMORE,
                       ST_FQ_EMPTYLINES, ST_FQ_LENMISMATCH, ST_DONTCARE};
  for (int rc : {0, EFORMAT})
    for (u32 flags : {0u, 1u, 4u, 8u, 2u, 5u, 16u})
      for (u32 code : codes)
        for (bool last : {false, true})
          for (bool ring : {false, true})
            for (u64 row_base : {0ull, 1ull})
              for (u64 count : {0ull, 1ull, 7ull}) {  // below / at / above row_base
                DevResult dr{};
                dr.count = count;
                dr.flags = flags;
                dr.code = code;
                const SlabOutcome got = classify(rc, dr, row_base, last, ring);
                CHECK(got == expect_outcome(rc, flags, code, count, row_base, last, ring));
                if (!ring) CHECK(got == SlabOutcome::Clean || got == SlabOutcome::FallBack);
                if (got != SlabOutcome::FallBack) CHECK(rc == 0 && count >= row_base);
              }
  DevResult dr{};
  dr.count = 5;
  dr.code = ST_FQ_TRUNC;
  CHECK(classify(0, dr, 1, true, true) == SlabOutcome::GoError);
  CHECK(classify(0, dr, 1, false, true) == SlabOutcome::FallBack);
  CHECK(classify(0, dr, 1, true, false) == SlabOutcome::FallBack);
  dr.code = ST_NEEDMORE;
  dr.flags = RF_HALO;
  CHECK(classify(0, dr, 1, false, true) == SlabOutcome::Partial);
  CHECK(classify(0, dr, 1, true, true) == SlabOutcome::FallBack);
  CHECK(classify(0, dr, 1, false, false) == SlabOutcome::FallBack);
  dr.code = ST_END;
  dr.flags = 0;
  CHECK(classify(0, dr, 1, false, true) == SlabOutcome::Partial);
  CHECK(classify(0, dr, 1, false, false) == SlabOutcome::FallBack);
  CHECK(classify(0, dr, 1, true, true) == SlabOutcome::Clean);
  CHECK(classify(0, dr, 1, true, false) == SlabOutcome::Clean);
  CHECK(RF_CAPACITY == 1 && RF_INTERNAL == 2 && RF_HALO == 4 && RF_FIXQUEUE == 8 && RF_MISSPEC == 16);
}

static void test_row_cursor() {
  RowCursor cur{10, 100, 0};
  const u64 a[] = {100, 20, 120, 30};  // rows {off, len}
  CHECK(cur.accept(a, 2, true));
  CHECK(cur.total == 12 && cur.next_off == 150 && cur.last_len == 30);
  const u64 gap[] = {151, 5};  // a first chunk that does not start at next_off is refused
  CHECK(!cur.accept(gap, 1, true));
  CHECK(cur.total == 12 && cur.next_off == 150 && cur.last_len == 30);
  CHECK(cur.accept(gap, 1, false));  // a later chunk of a slab is not seam-checked
  CHECK(cur.total == 13 && cur.next_off == 156 && cur.last_len == 5);
  CHECK(cur.accept(nullptr, 0, true));  // a slab that owns no rows
  CHECK(cur.total == 13 && cur.next_off == 156 && cur.last_len == 5);
  const u64 empty_last[] = {156, 4, 160, 0};
  CHECK(cur.accept(empty_last, 2, true) && cur.last_len == 0 && cur.next_off == 160 && cur.total == 15);
}

static void test_table_end() {
  std::vector<uint8_t> f;
  int reads = 0;
  auto byte_at = [&](u64 off, uint8_t *b) {
    ++reads;
    if (off >= f.size()) return false;
    *b = f[off];
    return true;
  };
  auto unreadable = [](u64, uint8_t *) { return false; };
  f.assign({'@', 'a', '\n', 'A', '\n', '+', '\n', 'I', '\n', '\n', '\n'});  // one record, a blank tail
  const u64 end = f.size();
  CHECK(table_ends_at_file_end(F_FASTQ, 9, end, 9, byte_at));    // both bytes are '\n'
  CHECK(table_ends_at_file_end(F_FASTQ, end, end, 9, byte_at));  // the table ends at the file end
  CHECK(!table_ends_at_file_end(F_FASTQ, end + 1, end, 9, byte_at));
  CHECK(!table_ends_at_file_end(F_FASTQ, 7, end, 9, byte_at));   // f[7] = 'I'
  f[end - 1] = 'x';
  CHECK(!table_ends_at_file_end(F_FASTQ, 9, end, 9, byte_at));   // the file does not end in '\n'
  f[end - 1] = '\n';
  CHECK(!table_ends_at_file_end(F_FASTQ, 9, end, 9, unreadable));  // a failed read is a violation
  reads = 0;
  CHECK(table_ends_at_file_end(F_FASTQ, end, end, 9, unreadable) && reads == 0);
  // FASTA and line tables consume every byte
  CHECK(!table_ends_at_file_end(F_FASTA, 9, end, 3, byte_at));
  CHECK(table_ends_at_file_end(F_FASTA, end, end, 3, byte_at));
  CHECK(!table_ends_at_file_end(F_LINE, 9, end, 0, byte_at));
  // the line index's last row is the bytes after the last '\n': not empty, the file cannot end in '\n'
  CHECK(!table_ends_at_file_end(F_LINE, end, end, 1, byte_at));
  CHECK(table_ends_at_file_end(F_LINE, end, end, 0, byte_at));
  CHECK(!table_ends_at_file_end(F_LINE, end, end, 1, unreadable));
  f[end - 1] = 'x';
  CHECK(table_ends_at_file_end(F_LINE, end, end, 1, byte_at));
}

int main() {
  test_layout();
  test_ring_slab_bytes();
  test_classify();
  test_row_cursor();
  test_table_end();
  if (failures) {
    printf("slabwalk_test: %d checks failed\n", failures);
    return 1;
  }
  printf("slabwalk_test ok\n");
  return 0;
}
