// bwgr_amd/csrc/devbufs.h -- the holder that owns device arrays, streams and events, and releases them when it goes away.  Plain C++17: the
// device runtime is the backend B (bwgr_hip.hip has the HIP one, tests/devbufs_check.cpp a counting fake), which provides
//   stream_t, event_t                                    handle types, value-initialised = none
//   void *alloc(size_t bytes), void free(void *)         alloc: nullptr where it fails, and no error left pending in the runtime
//   bool stream_create(stream_t *, unsigned flags, int priority), void stream_sync(stream_t), void stream_destroy(stream_t)
//        (priority 0 is the runtime's default priority: a backend may create such a stream without naming one)
//   bool event_create(event_t *, unsigned flags), void event_destroy(event_t)
// and keeps the process-wide counts of what is alive.
// A per-call holder frees the call's temporaries on every path out of the scope; given a stream, it waits for that stream first, so that no
// kernel or asynchronous copy still uses a buffer or a host local of the frame that goes away (a host vector that is copied from asynchronously
// is declared before the holder, and so outlives that wait).  A handle's holder is a member of the handle: the handle's typed pointers are
// aliases of what the holder owns, and deleting the handle releases all of it.
// Beside the holder: EventPairs, a chain's pool of timing pairs, whose events are the chain's holder's.
#pragma once
#include <stddef.h>
#include <algorithm>
#include <initializer_list>
#include <vector>

namespace bwgr {
template <class B> class DevHolder {
 public:
  using stream_t = typename B::stream_t;
  using event_t = typename B::event_t;
  // one member of a group for take(): {&pointer, bytes}, want_stream(&s, flags, priority) or want_event(&e, flags)
  struct Want {
    enum Kind { ARRAY, STREAM, EVENT } kind;
    void *dst; void (*set)(void *dst, void *q);
    size_t bytes; unsigned flags; int priority;
    template <typename T> Want(T **p, size_t bytes_)
        : kind(ARRAY), dst(p), set([](void *d, void *q) { *static_cast<T **>(d) = static_cast<T *>(q); }), bytes(bytes_), flags(0), priority(0) {}
    Want(Kind k, void *d, unsigned f, int pr) : kind(k), dst(d), set(nullptr), bytes(0), flags(f), priority(pr) {}
  };
  static Want want_stream(stream_t *s, unsigned flags, int priority) { return Want(Want::STREAM, s, flags, priority); }
  static Want want_event(event_t *e, unsigned flags) { return Want(Want::EVENT, e, flags, 0); }

  DevHolder() = default;
  explicit DevHolder(stream_t st) : sync_stream_(st), sync_(true) {}
  DevHolder(const DevHolder &) = delete;
  DevHolder &operator=(const DevHolder &) = delete;
  // events, then the owned streams (each once its work is done), then the arrays: nothing enqueued still reads an array that goes
  ~DevHolder() {
    if (sync_) B::stream_sync(sync_stream_);
    release(0, 0, 0);
  }

  // count elements of T (at least one byte-sized allocation: count == 0 still gives a pointer); nullptr where the allocation fails
  template <typename T> T *get(size_t count) {
    void *q = B::alloc(sizeof(T) * (count ? count : 1));
    if (q) arrays_.push_back(q); else failed_ = true;
    return static_cast<T *>(q);
  }
  // whether any get() of this holder, one inside take() included, has returned nullptr: a call makes the gets of a group and asks once
  bool failed() const { return failed_; }
  stream_t stream(unsigned flags, int priority) {
    stream_t s{};
    if (!B::stream_create(&s, flags, priority)) return stream_t{};
    streams_.push_back(s);
    return s;
  }
  event_t event(unsigned flags) {
    event_t e{};
    if (!B::event_create(&e, flags)) return event_t{};
    events_.push_back(e);
    return e;
  }
  // All or nothing: every destination is set and owned, or every one is null and nothing of this call stays allocated.  What a handle
  // allocates lazily as a group goes through here, so that the group's first pointer does say whether the group exists.
  bool take(std::initializer_list<Want> wants) {
    const size_t na = arrays_.size(), ns = streams_.size(), ne = events_.size();
    bool ok = true;
    for (const Want &w : wants) {
      if (w.kind == Want::ARRAY) { void *q = get<unsigned char>(w.bytes); w.set(w.dst, q); ok = q != nullptr; }
      else if (w.kind == Want::STREAM) ok = (*static_cast<stream_t *>(w.dst) = stream(w.flags, w.priority)) != stream_t{};
      else ok = (*static_cast<event_t *>(w.dst) = event(w.flags)) != event_t{};
      if (!ok) break;
    }
    if (ok) return true;
    release(na, ns, ne);   // (nothing was enqueued on a stream of this call)
    for (const Want &w : wants) {
      if (w.kind == Want::ARRAY) w.set(w.dst, nullptr);
      else if (w.kind == Want::STREAM) *static_cast<stream_t *>(w.dst) = stream_t{};
      else *static_cast<event_t *>(w.dst) = event_t{};
    }
    return false;
  }
  // frees one owned array early; a pointer this holder does not own (nullptr too) is left alone
  void drop(void *q) {
    auto it = std::find(arrays_.begin(), arrays_.end(), q);
    if (q && it != arrays_.end()) { B::free(q); arrays_.erase(it); }
  }

 private:
  // releases what was taken after the first na arrays, ns streams and ne events, the last taken first
  void release(size_t na, size_t ns, size_t ne) {
    for (; events_.size() > ne; events_.pop_back()) B::event_destroy(events_.back());
    for (; streams_.size() > ns; streams_.pop_back()) { B::stream_sync(streams_.back()); B::stream_destroy(streams_.back()); }
    for (; arrays_.size() > na; arrays_.pop_back()) B::free(arrays_.back());
  }
  std::vector<void *> arrays_;
  std::vector<stream_t> streams_;
  std::vector<event_t> events_;
  stream_t sync_stream_{};
  bool sync_ = false;
  bool failed_ = false;
};

// A pool of event pairs for timing (flags 0), one pair around each launch since the last fold.  It owns nothing: every event is a holder's,
// made the first time its slot is reached and reused after every rewind(), so a launch creates and destroys nothing and no path out of a
// caller has anything to clean up.  next() hands out the first unused pair, commit() marks it used once the launches it times stand; a pair
// that is not committed is the next one handed out.
template <class B> class EventPairs {
 public:
  using event_t = typename B::event_t;
  static constexpr size_t kCapacity = 2048;   // pairs: a caller folds (reads the pairs, rewinds) once full()
  // false, with both outputs empty, where the pool is full or the slot's pair cannot be made (nothing of it stays behind)
  bool next(DevHolder<B> &own, event_t *e0, event_t *e1) {
    *e0 = *e1 = event_t{};
    if (full()) return false;
    if (2 * used_ == ev_.size()) {
      event_t a{}, b{};
      if (!own.take({DevHolder<B>::want_event(&a, 0), DevHolder<B>::want_event(&b, 0)})) return false;
      ev_.push_back(a); ev_.push_back(b);
    }
    *e0 = ev_[2 * used_]; *e1 = ev_[2 * used_ + 1];
    return out_ = true;
  }
  void commit() { if (out_) { ++used_; out_ = false; } }   // (the pair last handed out, once)
  size_t used() const { return used_; }
  void pair(size_t i, event_t *e0, event_t *e1) const { *e0 = ev_[2 * i]; *e1 = ev_[2 * i + 1]; }
  void rewind() { used_ = 0; out_ = false; }
  bool full() const { return used_ >= kCapacity; }

 private:
  std::vector<event_t> ev_;   // aliases of the holder's events: slot i is ev_[2 i], ev_[2 i + 1]
  size_t used_ = 0;
  bool out_ = false;          // a pair was handed out and is neither committed nor rewound
};
}  // namespace bwgr
