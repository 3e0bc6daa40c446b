// sidx_devbuf.hpp -- the two pieces of host bookkeeping every entry point shares: the error sink
// (one view over the status / err_len / err fields of either result struct) and the context's
// device caches (typed buffers that register with one owner, which counts, trims and frees
// them).  Policy only: no HIP here -- the allocator comes in as a DevAlloc (sidx_host.hpp binds
// dev_malloc / hipFree; tests/host/devbuf_test.cpp binds malloc / free).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>
#include <string>

#include "../../include/shockidx.h"

namespace sidx_host {

// ---- the error sink ----------------------------------------------------------------------------
// Where an error goes: the three fields shockidx_result and shockidx_subset_result share.  A null
// view (no result, nullptr) discards the text; the code is still returned.
struct Err {
  int32_t *status = nullptr;
  uint64_t *err_len = nullptr;
  char *err = nullptr;
  Err() {}
  Err(decltype(nullptr)) {}
  template <class R> Err(R *r) {
    if (r) {
      static_assert(sizeof r->err == 256, "result error text");
      status = &r->status;
      err_len = &r->err_len;
      err = r->err;
    }
  }
};
constexpr size_t ERR_TEXT_MAX = 255;  // bytes of text a result holds (+ a NUL)

// Length-based (the FASTA message embeds raw file bytes, NULs included): at most ERR_TEXT_MAX
// bytes and a NUL; err_len is the bytes kept.  Returns code.
inline int set_msg(Err e, int code, const char *msg, size_t len) {
  if (e.err) {
    const size_t k = len < ERR_TEXT_MAX ? len : ERR_TEXT_MAX;
    memmove(e.err, msg, k);
    e.err[k] = 0;
    *e.err_len = k;
    *e.status = code;
  }
  return code;
}
inline int set_msg(Err e, int code, const char *msg) { return set_msg(e, code, msg, strlen(msg)); }
inline int set_msg(Err e, int code, const std::string &m) { return set_msg(e, code, m.data(), m.size()); }
// one result's error into another: its err_len bytes, under `code`
template <class R> int forward_error(Err to, const R &from, int code) {
  return set_msg(to, code, from.err, (size_t)from.err_len);
}

// ---- device buffers ----------------------------------------------------------------------------
// How device memory is had: alloc returns 0 or an error number errstr() turns into text; node
// asks for memory the tile passes stream (dev_malloc in sidx_host.hpp).
struct DevAlloc {
  int (*alloc)(void **p, size_t bytes, bool node);
  void (*release)(void *p);
  const char *(*errstr)(int e);
};

enum class BufClass {
  Large,  // dropped by any trim that has to act
  Tile,   // the per-tile words: dropped only by a trim to 0, or when the rest is still over `keep`
};

class BufSet;

// One device allocation of the set: the pointer, its capacity in elements and what a trim may
// do with it.  The typed face is DevBuf<T> below.
class DevBufBase {
 public:
  DevBufBase(const DevBufBase &) = delete;
  DevBufBase &operator=(const DevBufBase &) = delete;
  ~DevBufBase() { drop(); }
  uint64_t cap = 0;   // elements held (0: none)
  bool node = false;  // allocate as node memory
  uint64_t bytes() const { return cap * elem_; }  // what the set counts (slack excluded)
  void drop();
  // Grow-only: at least `need` elements afterwards.  Enough already: nothing happens.  Else the
  // old block is freed first and need + need/8 + 64 elements (+ 64 bytes of slack) allocated.
  int ensure(uint64_t need, Err res) {
    if (cap >= need && p_) return 0;
    return alloc(need + need / 8 + 64, 64, res);
  }
  // Exact size: exactly n elements afterwards, reallocated whenever n differs from what is held.
  int exact(uint64_t n, Err res) {
    if (cap == n && p_) return 0;
    return alloc(n, 0, res);
  }

 protected:
  DevBufBase(BufSet &set, size_t elem, BufClass cls, bool node_mem, const char *what);
  int alloc(uint64_t n, size_t slack, Err res);
  void *p_ = nullptr;

 private:
  friend class BufSet;
  BufSet &set_;
  const size_t elem_;
  const BufClass cls_;
  const char *const what_;  // the allocation's name in its error text
  DevBufBase *next_ = nullptr;
};

// The context's device caches.  Buffers register on construction (declare the set before them);
// counting, trimming and the final free walk that list, so a new cache is one declaration.
class BufSet {
 public:
  explicit BufSet(const DevAlloc *a) : alloc_(a) {}
  BufSet(const BufSet &) = delete;
  BufSet &operator=(const BufSet &) = delete;
  uint64_t bytes() const {
    uint64_t b = 0;
    for (const DevBufBase *d = head_; d; d = d->next_) b += d->bytes();
    return b;
  }
  void drop(BufClass cls) {
    for (DevBufBase *d = head_; d; d = d->next_)
      if (d->cls_ == cls) d->drop();
  }
  void drop_all() {
    for (DevBufBase *d = head_; d; d = d->next_) d->drop();
  }
  // Free down to `keep` bytes.  At or under it: nothing happens (false).  Else quiesce() (the
  // device may still be reading them), every large buffer goes, and the tile block too when
  // keep is 0 or the rest is still over it -- a fresh, zeroed status array then comes back with
  // the next build.
  template <class Quiesce> bool trim(uint64_t keep, Quiesce quiesce) {
    if (bytes() <= keep) return false;
    quiesce();
    drop(BufClass::Large);
    if (keep == 0 || bytes() > keep) drop(BufClass::Tile);
    return true;
  }
  // An exact-size workspace: each listed buffer holds exactly its n elements afterwards.  All do
  // already: nothing is trimmed or allocated.  Else everything goes first (trim to 0: the caches
  // of other builds), then each is allocated in list order; the first failure is returned, the
  // ones before it held, it and the ones after it empty.
  struct Want {
    DevBufBase *buf;
    uint64_t n;
  };
  template <class Quiesce> int exact(std::initializer_list<Want> want, Quiesce quiesce, Err res) {
    bool held = true;
    for (const Want &w : want) held = held && w.buf->cap == w.n;
    if (held) return 0;
    trim(0, quiesce);
    for (const Want &w : want)
      if (int rc = w.buf->exact(w.n, res)) return rc;
    return 0;
  }

 private:
  friend class DevBufBase;
  const DevAlloc *const alloc_;
  DevBufBase *head_ = nullptr;
};

inline DevBufBase::DevBufBase(BufSet &set, size_t elem, BufClass cls, bool node_mem, const char *what)
    : node(node_mem), set_(set), elem_(elem), cls_(cls), what_(what), next_(set.head_) {
  set.head_ = this;
}
inline void DevBufBase::drop() {
  if (p_) set_.alloc_->release(p_);
  p_ = nullptr;
  cap = 0;
}
inline int DevBufBase::alloc(uint64_t n, size_t slack, Err res) {
  drop();
  if (const int e = set_.alloc_->alloc(&p_, n * elem_ + slack, node)) {
    p_ = nullptr;
    char msg[ERR_TEXT_MAX + 1];
    snprintf(msg, sizeof msg, "%s: %s", what_, set_.alloc_->errstr(e));
    return set_msg(res, SHOCKIDX_EHIP, msg);
  }
  cap = n;
  return 0;
}

// A cache of T's whose capacity counts elements of PER T's each (the row table: two u64 words
// per row).  Converts to T* where the pointer is wanted; as<U>() for the carved workspaces.
template <class T, size_t PER = 1> class DevBuf : public DevBufBase {
 public:
  explicit DevBuf(BufSet &set, BufClass cls = BufClass::Large, bool node_mem = false, const char *what = "hipMalloc")
      : DevBufBase(set, PER * sizeof(T), cls, node_mem, what) {}
  T *get() const { return (T *)p_; }
  operator T *() const { return (T *)p_; }
  template <class U> U *as() const { return (U *)p_; }
};

}  // namespace sidx_host
