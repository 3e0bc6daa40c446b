// devbuf_test.cpp -- CPU test of the host bookkeeping in shock_amd/csrc/sidx_devbuf.hpp: the
// device-buffer set (growth, exact-size slots and sets, the tile block, trims, the final free) over a fake
// allocator, and the error sink over both result structs.  Stand-alone: it includes that header
// only, links nothing of the library and makes no HIP call.  The fake allocator is malloc / free,
// so a double free or a leak is a sanitizer report.  Built with the host sanitizers by
// `make -C shock_amd/csrc devbuf_test`; exit 0 = every check held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "sidx_devbuf.hpp"

using namespace sidx_host;
typedef uint64_t u64;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                \
    }                                                            \
  } while (0)

// ---- the fake allocator ------------------------------------------------------------------------
static int n_alloc = 0, n_free = 0, n_node = 0;
static size_t last_bytes = 0;
static bool fail_next = false;
static int fake_alloc(void **p, size_t bytes, bool node) {
  if (fail_next) {
    fail_next = false;
    return 2;
  }
  *p = malloc(bytes);
  ++n_alloc;
  n_node += node;
  last_bytes = bytes;
  return *p ? 0 : 2;
}
static void fake_release(void *p) {
  free(p);
  ++n_free;
}
static const char *fake_errstr(int e) { return e == 2 ? "out of memory" : "unknown"; }
static const DevAlloc FAKE = {fake_alloc, fake_release, fake_errstr};

// a context's worth of caches: two large ones, the slots, the tile block
struct Caches {
  BufSet bufs{&FAKE};
  DevBuf<uint8_t> in{bufs, BufClass::Large, true};
  DevBuf<u64, 2> rows{bufs};
  DevBuf<uint8_t> slot[2] = {DevBuf<uint8_t>{bufs, BufClass::Large, true, "hipMalloc(slab slot)"},
                             DevBuf<uint8_t>{bufs, BufClass::Large, true, "hipMalloc(slab slot)"}};
  DevBuf<u64> status{bufs, BufClass::Tile}, detail{bufs, BufClass::Tile}, fix{bufs, BufClass::Tile};
  // the tile block for `tiles` tiles: 7 + 4 + 4 words each, as ensure_tiles holds it
  int tiles(u64 tiles, Err res) {
    if (int rc = status.exact(7 * tiles, res)) return rc;
    if (int rc = detail.exact(4 * tiles, res)) return rc;
    return fix.exact(4 * tiles, res);
  }
  int quiesced = 0;
  bool trim(u64 keep) { return bufs.trim(keep, [this] { ++quiesced; }); }
};

static void test_growth() {
  Caches c;
  shockidx_result r;
  memset(&r, 0, sizeof r);
  CHECK(c.bufs.bytes() == 0 && !c.rows && c.rows.cap == 0);
  const int a0 = n_alloc, f0 = n_free;
  CHECK(c.rows.ensure(1000, &r) == 0);
  const u64 want = 1000 + 1000 / 8 + 64;
  CHECK(c.rows.cap == want && c.rows.get() != nullptr);
  CHECK(last_bytes == want * 16 + 64);  // two u64 per element, 64 bytes of slack
  CHECK(c.rows.bytes() == want * 16 && c.bufs.bytes() == want * 16);  // the slack is not counted
  CHECK(n_alloc == a0 + 1 && n_free == f0);
  u64 *p = c.rows;
  p[2 * (want - 1) + 1] = 7;  // the last element is there (typed access, ASan checks the bound)
  // at or below the capacity: the same pointer, nothing allocated
  CHECK(c.rows.ensure(want, &r) == 0 && c.rows.ensure(1, &r) == 0 && c.rows.ensure(0, &r) == 0);
  CHECK(c.rows.get() == p && n_alloc == a0 + 1 && n_free == f0 && c.rows.cap == want);
  // past it: freed first, then the formula again
  CHECK(c.rows.ensure(want + 1, &r) == 0);
  CHECK(c.rows.cap == want + 1 + (want + 1) / 8 + 64 && n_alloc == a0 + 2 && n_free == f0 + 1);
  // a byte buffer of node memory
  const int nn = n_node;
  CHECK(c.in.ensure(5, &r) == 0 && c.in.cap == 69 && last_bytes == 69 + 64 && n_node == nn + 1);
  CHECK(c.bufs.bytes() == c.rows.bytes() + 69);
  CHECK(r.status == 0 && r.err_len == 0);
}

template <class R> static void test_failed_alloc() {
  Caches c;
  R r;
  memset(&r, 0, sizeof r);
  CHECK(c.in.ensure(100, &r) == 0);
  const int a0 = n_alloc, f0 = n_free;
  fail_next = true;
  CHECK(c.in.ensure(100000, &r) == SHOCKIDX_EHIP);
  CHECK(!c.in && c.in.cap == 0 && c.bufs.bytes() == 0);  // empty
  CHECK(n_alloc == a0 && n_free == f0 + 1);              // the old block went exactly once
  CHECK(r.status == SHOCKIDX_EHIP && !strcmp(r.err, "hipMalloc: out of memory") && r.err_len == strlen(r.err));
  CHECK(strncmp(r.err, "hipMalloc: ", 11) == 0);
  // and it comes back
  CHECK(c.in.ensure(10, &r) == 0 && c.in.cap == 75 && n_free == f0 + 1);
  // a named allocation's text; a discarded one still returns the code
  fail_next = true;
  CHECK(c.slot[0].exact(4096, &r) == SHOCKIDX_EHIP && !strcmp(r.err, "hipMalloc(slab slot): out of memory"));
  fail_next = true;
  CHECK(c.slot[0].exact(4096, nullptr) == SHOCKIDX_EHIP && !c.slot[0]);
}

static void test_trim() {
  Caches c;
  CHECK(c.in.ensure(100000, nullptr) == 0 && c.rows.ensure(1000, nullptr) == 0 && c.tiles(80, nullptr) == 0);
  const u64 tile_bytes = 15 * 8 * 80, total = c.bufs.bytes();
  CHECK(c.status.bytes() + c.detail.bytes() + c.fix.bytes() == tile_bytes);
  CHECK(total == tile_bytes + c.in.bytes() + c.rows.bytes() && total > 2 * tile_bytes);
  // keep >= the total: nothing changes
  const int f0 = n_free;
  const void *pin = c.in.get();
  CHECK(!c.trim(total) && !c.trim(total + 1) && c.quiesced == 0);
  CHECK(c.bufs.bytes() == total && c.in.get() == pin && n_free == f0);
  // between the tile block's size and the total: the large buffers go, the tile block stays
  const void *pst = c.status.get();
  CHECK(c.trim(total - 1) && c.quiesced == 1);
  CHECK(!c.in && !c.rows && c.in.cap == 0 && c.rows.cap == 0 && n_free == f0 + 2);
  CHECK(c.status.get() == pst && c.detail && c.fix && c.bufs.bytes() == tile_bytes);
  CHECK(!c.trim(tile_bytes) && c.quiesced == 1);  // now at keep: nothing to do
  // below the tile block's size: the tile block goes too
  CHECK(c.in.ensure(100000, nullptr) == 0);
  CHECK(c.trim(tile_bytes - 1) && c.quiesced == 2);
  CHECK(c.bufs.bytes() == 0 && !c.in && !c.status && !c.detail && !c.fix && c.fix.cap == 0);
  // keep = 0: everything, the tile block included
  CHECK(c.in.ensure(10, nullptr) == 0 && c.tiles(8, nullptr) == 0 && c.slot[0].exact(64, nullptr) == 0);
  const int f1 = n_free;
  CHECK(c.trim(0) && c.bufs.bytes() == 0 && n_free == f1 + 5);
  CHECK(!c.in && !c.status && !c.detail && !c.fix && !c.slot[0]);
  CHECK(!c.trim(0));  // empty: nothing to do
  // a tile block alone under a non-zero keep it exceeds
  CHECK(c.tiles(8, nullptr) == 0 && c.trim(1) && c.bufs.bytes() == 0);
}

static void test_slots() {
  Caches c;
  const int a0 = n_alloc, f0 = n_free;
  for (auto &s : c.slot) CHECK(s.exact(5000, nullptr) == 0);
  CHECK(n_alloc == a0 + 2 && last_bytes == 5000);  // exact: no growth, no slack
  CHECK(c.slot[0].cap == 5000 && c.slot[1].cap == 5000 && c.bufs.bytes() == 2 * 5000);  // counted twice
  const void *p0 = c.slot[0].get(), *p1 = c.slot[1].get();
  for (auto &s : c.slot) CHECK(s.exact(5000, nullptr) == 0);  // the same size: nothing allocated
  CHECK(n_alloc == a0 + 2 && n_free == f0 && c.slot[0].get() == p0 && c.slot[1].get() == p1);
  for (auto &s : c.slot) CHECK(s.exact(4000, nullptr) == 0);  // another size, smaller too: both again
  CHECK(n_alloc == a0 + 4 && n_free == f0 + 2 && c.bufs.bytes() == 2 * 4000);
  // the second slot fails: the first is held and counted, nothing is lost track of
  for (auto &s : c.slot) s.drop();
  CHECK(c.slot[0].exact(100, nullptr) == 0);
  fail_next = true;
  CHECK(c.slot[1].exact(100, nullptr) == SHOCKIDX_EHIP);
  CHECK(c.bufs.bytes() == 100 && c.trim(0) && c.bufs.bytes() == 0);
}

// the exact-size workspace of a slab walk (BufSet::exact)
static void test_exact_set() {
  Caches c;
  shockidx_result r;
  memset(&r, 0, sizeof r);
  auto quiesce = [&] { ++c.quiesced; };
  // from nothing: each buffer allocated in list order (the slots first), nothing to drop
  const int a0 = n_alloc, f0 = n_free;
  CHECK(c.bufs.exact({{&c.slot[0], 5000}, {&c.slot[1], 5000}, {&c.rows, 100}}, quiesce, &r) == 0);
  CHECK(n_alloc == a0 + 3 && n_free == f0 && c.quiesced == 0 && last_bytes == 100 * 16);  // (the rows came last)
  CHECK(c.slot[0].cap == 5000 && c.slot[1].cap == 5000 && c.rows.cap == 100 && c.bufs.bytes() == 2 * 5000 + 1600);
  // every size matches: no free, no allocation, no quiesce -- the caches of other builds stay too
  CHECK(c.in.ensure(10, &r) == 0 && c.tiles(8, &r) == 0);
  const int a1 = n_alloc, f1 = n_free;
  const void *p0 = c.slot[0].get(), *pr = c.rows.get(), *pin = c.in.get();
  CHECK(c.bufs.exact({{&c.slot[0], 5000}, {&c.slot[1], 5000}, {&c.rows, 100}}, quiesce, &r) == 0);
  CHECK(n_alloc == a1 && n_free == f1 && c.quiesced == 0);
  CHECK(c.slot[0].get() == p0 && c.rows.get() == pr && c.in.get() == pin && c.status);
  // one size differs: everything is dropped first (the other caches and the tile block with it),
  // then each listed buffer is allocated, in list order, to exactly its size
  static size_t order[4];
  static int n_order;
  n_order = 0;
  const DevAlloc logging = {[](void **p, size_t bytes, bool node) {
                              if (n_order < 4) order[n_order++] = bytes;
                              return fake_alloc(p, bytes, node);
                            },
                            fake_release, fake_errstr};
  {
    BufSet set(&logging);
    DevBuf<uint8_t> a{set}, b{set}, other{set};
    DevBuf<u64> tile{set, BufClass::Tile};
    DevBuf<u64, 2> rows{set};
    int q = 0;
    CHECK(set.exact({{&a, 300}, {&b, 300}, {&rows, 7}}, [&] { ++q; }, &r) == 0 && q == 0);
    CHECK(other.ensure(50, &r) == 0 && tile.exact(9, &r) == 0);
    n_order = 0;
    const int a2 = n_alloc, f2 = n_free;
    bool quiesced_first = false;  // (before anything is freed)
    auto before_drop = [&] { ++q; quiesced_first = n_alloc == a2 && n_free == f2; };
    CHECK(set.exact({{&a, 300}, {&b, 300}, {&rows, 8}}, before_drop, &r) == 0);
    CHECK(quiesced_first && q == 1 && n_free == f2 + 5 && n_alloc == a2 + 3);  // all five went, three came back
    CHECK(n_order == 3 && order[0] == 300 && order[1] == 300 && order[2] == 8 * 16);
    CHECK(a.cap == 300 && b.cap == 300 && rows.cap == 8 && !other && !tile && set.bytes() == 600 + 128);
    // an allocation fails midway: its error, the buffers before it held, it and the rest empty,
    // the count right -- and the next call starts over
    static int countdown;
    countdown = 2;
    const DevAlloc failing = {[](void **p, size_t bytes, bool node) { return --countdown == 0 ? 2 : fake_alloc(p, bytes, node); },
                              fake_release, fake_errstr};
    BufSet set2(&failing);
    DevBuf<uint8_t> s0{set2, BufClass::Large, true, "hipMalloc(slab slot)"}, s1{set2, BufClass::Large, true, "hipMalloc(slab slot)"};
    DevBuf<u64, 2> rows2{set2};
    CHECK(set2.exact({{&s0, 64}, {&s1, 64}, {&rows2, 4}}, [] {}, &r) == SHOCKIDX_EHIP);
    CHECK(r.status == SHOCKIDX_EHIP && !strcmp(r.err, "hipMalloc(slab slot): out of memory"));
    CHECK(s0 && s0.cap == 64 && !s1 && s1.cap == 0 && !rows2 && rows2.cap == 0 && set2.bytes() == 64);
    countdown = 100;
    CHECK(set2.exact({{&s0, 64}, {&s1, 64}, {&rows2, 4}}, [] {}, &r) == 0);
    CHECK(s0.cap == 64 && s1.cap == 64 && rows2.cap == 4 && set2.bytes() == 128 + 64);
  }
}

static void test_destroy() {
  const int a0 = n_alloc, f0 = n_free;
  {
    Caches c;
    CHECK(c.in.ensure(1, nullptr) == 0 && c.rows.ensure(1, nullptr) == 0 && c.tiles(3, nullptr) == 0);
    for (auto &s : c.slot) CHECK(s.exact(32, nullptr) == 0);
    CHECK(n_alloc == a0 + 7);
    c.bufs.drop_all();  // what shockidx_ctx_destroy does
    CHECK(n_free == f0 + 7 && c.bufs.bytes() == 0);
    c.bufs.drop_all();  // and again: nothing left to free
    CHECK(n_free == f0 + 7);
    CHECK(c.in.ensure(1, nullptr) == 0);  // left to the destructors
  }
  CHECK(n_alloc == a0 + 8 && n_free == f0 + 8);
}

// ---- the error sink ----------------------------------------------------------------------------
template <class R> static void test_sink() {
  R r;
  memset(&r, 0xEE, sizeof r);
  std::string big(300, 'x');
  big[254] = 'y';
  CHECK(set_msg(&r, SHOCKIDX_EIO, big) == SHOCKIDX_EIO);
  CHECK(r.status == SHOCKIDX_EIO && r.err_len == 255 && r.err[255] == 0 && strlen(r.err) == 255 && r.err[254] == 'y');
  CHECK(set_msg(&r, SHOCKIDX_EIO, big.c_str()) == SHOCKIDX_EIO && r.err_len == 255 && r.err[255] == 0);
  // set by length: an embedded NUL keeps every byte
  const char raw[] = "Invalid fasta entry: AC\0GT\n";
  CHECK(set_msg(&r, SHOCKIDX_EFORMAT, raw, sizeof raw - 1) == SHOCKIDX_EFORMAT);
  CHECK(r.status == SHOCKIDX_EFORMAT && r.err_len == sizeof raw - 1 && !memcmp(r.err, raw, sizeof raw));
  CHECK(strlen(r.err) == 23);
  // the C-string face stops at the NUL
  CHECK(set_msg(&r, SHOCKIDX_EFORMAT, raw) == SHOCKIDX_EFORMAT && r.err_len == 23);
  // a null sink is harmless, and the code still comes back
  CHECK(set_msg(nullptr, SHOCKIDX_EINVAL, "x") == SHOCKIDX_EINVAL);
  CHECK(set_msg((R *)nullptr, SHOCKIDX_EINVAL, big) == SHOCKIDX_EINVAL);
  CHECK(set_msg(Err(), SHOCKIDX_EINVAL, raw, sizeof raw - 1) == SHOCKIDX_EINVAL);
  CHECK(forward_error(nullptr, r, -3) == -3);
}

template <class From, class To> static void test_forward() {
  From a;
  To b;
  memset(&a, 0, sizeof a);
  memset(&b, 0xEE, sizeof b);
  const char raw[] = "Invalid fasta entry: \0>\0";
  set_msg(&a, SHOCKIDX_EFORMAT, raw, sizeof raw - 1);
  CHECK(forward_error(&b, a, a.status) == SHOCKIDX_EFORMAT);
  CHECK(b.status == a.status && b.err_len == a.err_len && b.err_len == sizeof raw - 1);
  CHECK(!memcmp(b.err, a.err, a.err_len + 1));
  // under another code, and a full-length text
  set_msg(&a, SHOCKIDX_EHIP, std::string(400, 'z'));
  CHECK(forward_error(&b, a, SHOCKIDX_EINTERNAL) == SHOCKIDX_EINTERNAL);
  CHECK(b.status == SHOCKIDX_EINTERNAL && b.err_len == 255 && !memcmp(b.err, a.err, 256));
}

int main() {
  test_growth();
  test_failed_alloc<shockidx_result>();
  test_failed_alloc<shockidx_subset_result>();
  test_trim();
  test_slots();
  test_exact_set();
  test_destroy();
  test_sink<shockidx_result>();
  test_sink<shockidx_subset_result>();
  test_forward<shockidx_result, shockidx_subset_result>();
  test_forward<shockidx_subset_result, shockidx_result>();
  test_forward<shockidx_result, shockidx_result>();
  CHECK(n_alloc == n_free);  // (LeakSanitizer has the last word at exit)
  if (failures) {
    printf("devbuf_test: %d check(s) failed\n", failures);
    return 1;
  }
  printf("devbuf_test ok\n");
  return 0;
}
