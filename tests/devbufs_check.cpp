// tests/devbufs_check.cpp -- the device holder (bwgr_amd/csrc/devbufs.h) on a counting fake backend that can fail the N-th allocation,
// stream creation or event creation; and the pool of timing pairs that takes its events from a holder.  A program of its own: built with -fsanitize=address,undefined and run by tests/test_devbufs_cpu.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <set>
#include <string>
#include <vector>
#include "../bwgr_amd/csrc/devbufs.h"

static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); ++g_failed; } } while (0)

struct FakeStream { int id; };
struct FakeEvent { int id; };
struct Fake {
  using stream_t = FakeStream *;
  using event_t = FakeEvent *;
  static inline int64_t live[3] = {0, 0, 0};
  static inline int fail_at[3] = {0, 0, 0};   // fail the N-th creation of that kind from now (1 = the next one); 0: never
  static inline std::set<void *> arrays, streams, events;   // what is alive: a double release is seen here before the sanitizer sees it
  static inline std::vector<std::string> log;
  static bool fails(int kind) { return fail_at[kind] > 0 && --fail_at[kind] == 0; }
  static void *alloc(size_t bytes) {
    if (bytes == 0 || fails(0)) return nullptr;
    void *q = malloc(bytes);
    arrays.insert(q); ++live[0];
    return q;
  }
  static void free(void *q) { CHECK(arrays.erase(q) == 1); --live[0]; ::free(q); log.push_back("free"); }
  static bool stream_create(stream_t *s, unsigned, int priority) {
    if (fails(1)) return false;
    *s = new FakeStream{priority};
    streams.insert(*s); ++live[1];
    return true;
  }
  static void stream_sync(stream_t s) { CHECK(s == nullptr || streams.count(s) == 1); log.push_back(s ? "sync" : "sync0"); }
  static void stream_destroy(stream_t s) { CHECK(streams.erase(s) == 1); --live[1]; delete s; log.push_back("sdestroy"); }
  static bool event_create(event_t *e, unsigned flags) {
    if (fails(2)) return false;
    *e = new FakeEvent{(int)flags};
    events.insert(*e); ++live[2];
    return true;
  }
  static void event_destroy(event_t e) { CHECK(events.erase(e) == 1); --live[2]; delete e; log.push_back("edestroy"); }
  static bool counts(int64_t a, int64_t s, int64_t e) { return live[0] == a && live[1] == s && live[2] == e; }
};
using Bufs = bwgr::DevHolder<Fake>;

// a group of k arrays, failing at every position in turn: all null, nothing kept, and the next take succeeds
static void arrays_fail_everywhere() {
  for (int k = 1; k <= 5; ++k)
    for (int pos = 1; pos <= k; ++pos) {
      Bufs h;
      double *keep = h.get<double>(3);   // something the holder already owns stays
      CHECK(keep && Fake::counts(1, 0, 0));
      double *a = nullptr; float *b = nullptr; int *c = nullptr; unsigned char *d = nullptr; uint16_t *e = nullptr;
      auto take = [&] {
        switch (k) {
          case 1: return h.take({{&a, 8}});
          case 2: return h.take({{&a, 8}, {&b, 40}});
          case 3: return h.take({{&a, 8}, {&b, 40}, {&c, 4}});
          case 4: return h.take({{&a, 8}, {&b, 40}, {&c, 4}, {&d, 1}});
          default: return h.take({{&a, 8}, {&b, 40}, {&c, 4}, {&d, 1}, {&e, 2}});
        }
      };
      // (stale values in the destinations: a failed take leaves none of them)
      a = keep;
      Fake::fail_at[0] = pos;
      CHECK(!take());
      CHECK(!a && !b && !c && !d && !e);
      CHECK(Fake::counts(1, 0, 0));
      CHECK(take());
      void *got[5] = {a, b, c, d, e};
      for (int i = 0; i < 5; ++i) CHECK((got[i] != nullptr) == (i < k));
      CHECK(Fake::counts(1 + k, 0, 0));
      a[0] = 1.0;   // (the array is there to be written)
      keep[2] = 2.0;
    }
  CHECK(Fake::counts(0, 0, 0));
}

// the draws group: one array, one stream, two events
static void mixed_fail_everywhere() {
  for (int pos = 1; pos <= 4; ++pos) {
    Bufs h;
    Fake::event_t before = h.event(0);
    CHECK(before && Fake::counts(0, 0, 1));
    double *draws = nullptr; Fake::stream_t st = nullptr; Fake::event_t ready = nullptr, freed = nullptr;
    auto take = [&] { return h.take({{&draws, 40}, Bufs::want_stream(&st, 1, 7), Bufs::want_event(&ready, 2), Bufs::want_event(&freed, 2)}); };
    if (pos == 1) Fake::fail_at[0] = 1;
    if (pos == 2) Fake::fail_at[1] = 1;
    if (pos >= 3) Fake::fail_at[2] = pos - 2;
    CHECK(!take());
    CHECK(!draws && !st && !ready && !freed);
    CHECK(Fake::counts(0, 0, 1));
    CHECK(take());
    CHECK(draws && st && ready && freed && ready != freed && st->id == 7 && ready->id == 2);
    CHECK(Fake::counts(1, 1, 3));
  }
  CHECK(Fake::counts(0, 0, 0));
}

static void get_stream_event() {
  Bufs h;
  Fake::fail_at[0] = 1;
  CHECK(h.get<double>(10) == nullptr && Fake::counts(0, 0, 0));
  int *z = h.get<int>(0);   // count == 0: still a pointer
  CHECK(z != nullptr && Fake::counts(1, 0, 0));
  Fake::fail_at[1] = 1;
  CHECK(h.stream(0, 0) == nullptr && Fake::counts(1, 0, 0));
  Fake::fail_at[2] = 1;
  CHECK(h.event(0) == nullptr && Fake::counts(1, 0, 0));
  CHECK(h.stream(0, 0) != nullptr && h.event(0) != nullptr && Fake::counts(1, 1, 1));
}

static void drop() {
  int other = 0;
  {
    Bufs h;
    float *a = h.get<float>(4), *b = h.get<float>(4), *c = h.get<float>(4);
    CHECK(a && b && c && Fake::counts(3, 0, 0));
    h.drop(b);
    CHECK(Fake::counts(2, 0, 0) && Fake::arrays.count(b) == 0);
    h.drop(b);         // no longer owned (a second free would fail the backend's check)
    h.drop(nullptr);
    h.drop(&other);    // never owned
    CHECK(Fake::counts(2, 0, 0));
    a[3] = c[3] = 1.0f;
  }
  CHECK(Fake::counts(0, 0, 0));
}

// failed(): false until a get returns null, one made inside take included; true from then on, whatever succeeds later
static void failure_latch() {
  for (int pos = 1; pos <= 3; ++pos) {
    Bufs h;
    CHECK(!h.failed());
    Fake::fail_at[0] = pos;
    for (int i = 1; i <= 4; ++i) {
      int *q = h.get<int>(2);
      CHECK((q == nullptr) == (i == pos));
      CHECK(h.failed() == (i >= pos));   // false before the failing get, true after it and after later successful ones
    }
    CHECK(Fake::counts(3, 0, 0));
  }
  {
    Bufs h;
    double *a = nullptr; int *b = nullptr;
    CHECK(h.take({{&a, 8}, {&b, 4}}) && !h.failed());
    Fake::fail_at[0] = 2;
    CHECK(!h.take({{&a, 8}, {&b, 4}}) && h.failed());
    CHECK(h.take({{&a, 8}, {&b, 4}}) && h.failed());
    Fake::fail_at[1] = 1;   // (a stream that cannot be made is no failed get)
    Bufs g;
    CHECK(g.stream(0, 0) == nullptr && !g.failed());
  }
  Bufs fresh;
  CHECK(!fresh.failed());
  CHECK(Fake::counts(0, 0, 0));
}

// events, then the owned streams (synchronised, then destroyed), then the arrays; the stream of a per-call holder is waited for first
static void fill(Bufs &h) {
  CHECK(h.get<int>(1) && h.stream(0, 0) && h.event(0) && h.get<int>(1) && h.event(0) && h.stream(0, 1));
  CHECK(Fake::counts(2, 2, 2));
  Fake::log.clear();
}
static void destruction_order() {
  const std::vector<std::string> release = {"edestroy", "edestroy", "sync", "sdestroy", "sync", "sdestroy", "free", "free"};
  FakeStream callers{0};
  Fake::streams.insert(&callers);
  { Bufs h; fill(h); }
  CHECK(Fake::log == release && Fake::counts(0, 0, 0));
  for (Fake::stream_t st : {&callers, (Fake::stream_t) nullptr}) {   // (the null stream is a stream too)
    { Bufs h(st); fill(h); }
    std::vector<std::string> want = release;
    want.insert(want.begin(), st ? "sync" : "sync0");
    CHECK(Fake::log == want && Fake::counts(0, 0, 0));
  }
  Fake::streams.erase(&callers);
}

// the pool of timing pairs: its events are the holder's, made once per slot and handed out again after rewind(); an uncommitted pair is
// the next one handed out; a pair that cannot be made leaves nothing behind; full() at exactly the capacity
using Pairs = bwgr::EventPairs<Fake>;
static void pairs_reuse() {
  {
    Bufs h;
    Pairs pool;
    Fake::event_t a0 = nullptr, a1 = nullptr, b0 = nullptr, b1 = nullptr, c0 = nullptr, c1 = nullptr;
    CHECK(pool.used() == 0 && !pool.full());
    CHECK(pool.next(h, &a0, &a1) && a0 && a1 && a0 != a1 && a0->id == 0 && a1->id == 0);   // (flags 0: timing enabled)
    CHECK(Fake::counts(0, 0, 2) && pool.used() == 0);                  // handed out is not yet used
    CHECK(pool.next(h, &b0, &b1) && b0 == a0 && b1 == a1);             // not committed: the same pair again, nothing new
    CHECK(Fake::counts(0, 0, 2));
    pool.commit();
    CHECK(pool.used() == 1);
    pool.commit();                                                     // (nothing handed out since: no second count)
    CHECK(pool.used() == 1);
    CHECK(pool.next(h, &b0, &b1) && b0 != a0 && b1 != a1 && b0 != b1 && Fake::counts(0, 0, 4));
    pool.commit();
    CHECK(pool.used() == 2);
    pool.pair(0, &c0, &c1); CHECK(c0 == a0 && c1 == a1);
    pool.pair(1, &c0, &c1); CHECK(c0 == b0 && c1 == b1);
    pool.rewind();
    CHECK(pool.used() == 0 && Fake::counts(0, 0, 4));                  // every event is kept
    pool.commit();                                                     // (made slots there are, but none handed out since the rewind)
    CHECK(pool.used() == 0);
    CHECK(pool.next(h, &c0, &c1) && c0 == a0); pool.rewind(); pool.commit();   // (a rewind takes a pair that is out back too)
    CHECK(pool.used() == 0);
    CHECK(pool.next(h, &c0, &c1) && c0 == a0 && c1 == a1); pool.commit();
    CHECK(pool.next(h, &c0, &c1) && c0 == b0 && c1 == b1); pool.commit();
    CHECK(Fake::counts(0, 0, 4) && pool.used() == 2);                  // made once, handed out again
    CHECK(pool.next(h, &c0, &c1) && c0 != b0 && Fake::counts(0, 0, 6));
  }
  CHECK(Fake::counts(0, 0, 0));
}
static void pairs_fail() {
  for (int pos = 1; pos <= 2; ++pos) {   // the first event of the pair, then the second
    Bufs h;
    Pairs pool;
    Fake::event_t keep = h.event(1), e0 = nullptr, e1 = nullptr, f0 = nullptr, f1 = nullptr;
    CHECK(pool.next(h, &e0, &e1)); pool.commit();
    CHECK(keep && Fake::counts(0, 0, 3));
    f0 = f1 = keep;   // (stale values: a failed next leaves none)
    Fake::fail_at[2] = pos;
    CHECK(!pool.next(h, &f0, &f1) && !f0 && !f1);
    CHECK(Fake::counts(0, 0, 3) && pool.used() == 1);
    CHECK(pool.next(h, &f0, &f1) && f0 && f1 && f0 != e0 && f1 != e1 && Fake::counts(0, 0, 5));
    pool.commit();
    CHECK(pool.used() == 2);
    pool.pair(0, &f0, &f1); CHECK(f0 == e0 && f1 == e1);
  }
  CHECK(Fake::counts(0, 0, 0));
}
static void pairs_capacity() {
  static_assert(Pairs::kCapacity == 2048, "the fold's cadence: once per 2048 sweeps");
  {
    Bufs h;
    Pairs pool;
    Fake::event_t e0 = nullptr, e1 = nullptr;
    for (size_t i = 0; i < Pairs::kCapacity; ++i) {
      CHECK(!pool.full());
      CHECK(pool.next(h, &e0, &e1));
      pool.commit();
    }
    CHECK(pool.full() && pool.used() == Pairs::kCapacity && Fake::counts(0, 0, 2 * (int64_t)Pairs::kCapacity));
    CHECK(!pool.next(h, &e0, &e1) && !e0 && !e1 && Fake::counts(0, 0, 2 * (int64_t)Pairs::kCapacity));   // a caller folds first
    pool.rewind();
    CHECK(!pool.full() && pool.next(h, &e0, &e1) && Fake::counts(0, 0, 2 * (int64_t)Pairs::kCapacity));
  }
  CHECK(Fake::counts(0, 0, 0));   // the holder went away: so did every event
}

int main() {
  pairs_reuse();
  pairs_fail();
  pairs_capacity();
  arrays_fail_everywhere();
  mixed_fail_everywhere();
  get_stream_event();
  drop();
  failure_latch();
  destruction_order();
  CHECK(Fake::arrays.empty() && Fake::streams.empty() && Fake::events.empty());
  if (g_failed) { fprintf(stderr, "devbufs_check: %d check(s) failed\n", g_failed); return 1; }
  printf("devbufs_check ok\n");
  return 0;
}
