// Host-only check of radtxfr_amd/csrc/rtx_devmem.h, built with -fsanitize=address,undefined by tests/test_devmem_host.py.
// "Device" memory is malloc here: the rtx_dev_* functions count live allocations, can be told to fail once, and name the
// "current device" of the calling thread.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <thread>

#include "../radtxfr_amd/csrc/rtx_devmem.h"

static std::atomic<long> g_live{0};  // allocations not yet freed
static bool g_fail_alloc = false;  // the next rtx_dev_alloc fails
static bool g_fail_copy = false;   // the next rtx_dev_h2d fails

int rtx_dev_alloc(void** p, size_t bytes) {
  *p = nullptr;
  if (g_fail_alloc) { g_fail_alloc = false; return 1; }
  *p = malloc(bytes ? bytes : 1);
  if (!*p) return 1;
  ++g_live;
  return 0;
}
void rtx_dev_free(void* p) {
  if (!p) return;
  --g_live;
  free(p);
}
int rtx_dev_h2d(void* d, const void* h, size_t bytes) {
  if (g_fail_copy) { g_fail_copy = false; return 1; }
  memcpy(d, h, bytes);
  return 0;
}
static thread_local int g_dev = 0;  // the calling thread's current device
int rtx_dev_current(int* dev) {
  *dev = g_dev;
  return 0;
}

static int g_bad = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) { fprintf(stderr, "%s:%d CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++g_bad; } \
  } while (0)

static void test_devbuf() {
  {
    DevBuf<double> b;
    CHECK(b.get() == nullptr && b.cap() == 0);
    CHECK(b.reserve(0) == 0 && b.get() == nullptr && g_live == 0);
    CHECK(b.reserve(10) == 0 && b.get() && b.cap() == 10 && g_live == 1);
    double* p10 = b.get();
    CHECK(b.reserve(4) == 0 && b.get() == p10 && b.cap() == 10);  // no shrink, no reallocation
    CHECK(b.reserve(10) == 0 && b.get() == p10);
    CHECK(b.reserve(100) == 0 && b.cap() == 100 && g_live == 1);  // growth frees the old array
    b.get()[99] = 1.0;                                            // the sanitizer checks the size
    // a failed allocation leaves (nullptr, 0); the old array is gone (freed first), and a later reserve succeeds
    g_fail_alloc = true;
    CHECK(b.reserve(1000) == 1 && b.get() == nullptr && b.cap() == 0 && g_live == 0);
    CHECK(b.reserve(1000) == 0 && b.cap() == 1000 && g_live == 1);
    // upload: reserve and copy
    const double h[3] = {1.0, 2.0, 3.0};
    DevBuf<double> u;
    CHECK(u.upload(h, 3) == 0 && u.cap() == 3 && u.get()[0] == 1.0 && u.get()[2] == 3.0 && g_live == 2);
    g_fail_copy = true;
    CHECK(u.upload(h, 3) == 1 && u.get() == nullptr && u.cap() == 0 && g_live == 1);
    g_fail_alloc = true;
    CHECK(u.upload(h, 3) == 1 && u.get() == nullptr && g_live == 1);
    CHECK(u.upload(h, 2) == 0 && u.cap() == 2 && g_live == 2);
    // move construction and move assignment: one owner, one free
    double* pu = u.get();
    DevBuf<double> m(std::move(u));
    CHECK(u.get() == nullptr && u.cap() == 0 && m.get() == pu && m.cap() == 2 && g_live == 2);
    b = std::move(m);  // b's 1000 elements are freed, m's array moves in
    CHECK(m.get() == nullptr && b.get() == pu && b.cap() == 2 && g_live == 1);
    b = std::move(b);  // self-move keeps the array
    CHECK(b.get() == pu && g_live == 1);
    b.reset();
    CHECK(b.get() == nullptr && b.cap() == 0 && g_live == 0);
    b.reset();  // twice is harmless
    CHECK(b.reserve(5) == 0 && g_live == 1);
  }
  CHECK(g_live == 0);  // the destructor freed the last one
}

static int g_builds = 0;
// a table of 4 doubles made from the key's first double
static int get_taps(DevTableCache<double>& c, int dev, double v, DevTableCache<double>::Hit* hit) {
  const double key[2] = {v, -v};
  return c.get(dev, key, sizeof(key), [&](std::vector<double>& h) { ++g_builds; h.assign(4, v); return 0; }, hit);
}

// as the library holds them: made with new, never destroyed, reachable to the end
static DevTableCache<double>* const cache = new DevTableCache<double>(16);
static DevTableCache<double>* const one = new DevTableCache<double>(0);

static void test_cache() {
  const double* first = nullptr;
  {
    DevTableCache<double>::Hit a;
    CHECK(get_taps(*cache, 0, 1.0, &a) == 0 && a.d && a.d[0] == 1.0 && a.d[3] == 1.0 && a.lock.owns_lock());
    CHECK(g_live == 1 && g_builds == 1);
    first = a.d;
    // the lock came back held: another thread cannot take the cache's mutex until it is released
    std::mutex* mu = a.lock.mutex();
    bool got = true;
    auto try_it = [&] { got = mu->try_lock(); if (got) mu->unlock(); };
    std::thread(try_it).join();
    CHECK(!got);
    a.lock.unlock();
    std::thread(try_it).join();
    CHECK(got);
  }
  {
    DevTableCache<double>::Hit a, b;
    CHECK(get_taps(*cache, 0, 1.0, &a) == 0 && a.d == first && g_builds == 1 && g_live == 1);  // equal bytes: a hit
    a.lock.unlock();
    CHECK(get_taps(*cache, 1, 1.0, &b) == 0 && b.d != first && g_builds == 2 && g_live == 2);  // another device: a miss
  }
  // failures insert nothing and free what they made
  {
    DevTableCache<double>::Hit a;
    const double key = 7.0;
    CHECK(cache->get(0, &key, sizeof(key), [&](std::vector<double>&) { return 1; }, &a) == 1 && !a.d && !a.lock.owns_lock());
    CHECK(g_live == 2);
    g_fail_alloc = true;
    CHECK(get_taps(*cache, 0, 7.0, &a) == 1 && g_live == 2 && !a.lock.owns_lock());
    g_fail_copy = true;
    CHECK(get_taps(*cache, 0, 7.0, &a) == 1 && g_live == 2);
    const int before = g_builds;
    CHECK(get_taps(*cache, 0, 7.0, &a) == 0 && g_builds == before + 1 && g_live == 3);  // it had not been inserted
  }
  // fill to 16 entries: (0,1) (1,1) (0,7) and 13 more
  for (int i = 0; i < 13; ++i) {
    DevTableCache<double>::Hit a;
    CHECK(get_taps(*cache, 0, 100.0 + i, &a) == 0);
  }
  CHECK(g_live == 16);
  {
    DevTableCache<double>::Hit a;
    const int before = g_builds;
    CHECK(get_taps(*cache, 0, 1.0, &a) == 0 && a.d == first && g_builds == before);  // the oldest is still there
    a.lock.unlock();
    CHECK(get_taps(*cache, 0, 999.0, &a) == 0 && g_builds == before + 1);  // the 17th distinct key evicts and frees it
    CHECK(g_live == 16);
    a.lock.unlock();
    CHECK(get_taps(*cache, 1, 1.0, &a) == 0 && g_builds == before + 1);  // the second oldest stayed
    a.lock.unlock();
    // a failure on a full cache evicts nothing
    g_fail_alloc = true;
    CHECK(get_taps(*cache, 0, 1.0, &a) == 1 && g_live == 16 && g_builds == before + 2);
    CHECK(get_taps(*cache, 1, 1.0, &a) == 0 && g_builds == before + 2);
    a.lock.unlock();
    CHECK(get_taps(*cache, 0, 1.0, &a) == 0 && a.d[0] == 1.0 && g_builds == before + 3 && g_live == 16);  // the evicted key again
  }
  // an empty key (one table per device) and an unbounded cache
  for (int i = 0; i < 40; ++i) {
    DevTableCache<double>::Hit a;
    CHECK(one->get(i % 20, nullptr, 0, [&](std::vector<double>& h) { h.assign(2, (double)i); return 0; }, &a) == 0);
    CHECK(a.d[0] == (double)(i % 20));
  }
  CHECK(g_live == 36);
}

// as the library holds it: made with new, never destroyed
static StreamScratch* const scratch = new StreamScratch();

static void test_stream_scratch() {
  const long live0 = g_live;
  int s1 = 0, s2 = 0;  // two "streams": any two distinct addresses, and the null stream
  void *a = nullptr, *b = nullptr, *c = nullptr, *d = nullptr, *p = nullptr;
  // distinct (device, stream) keys: distinct arrays, each at least as large as asked (the sanitizer checks the size)
  g_dev = 0;
  CHECK(scratch->get(&s1, 100, &a) == 0 && a && g_live == live0 + 1);
  CHECK(scratch->get(&s2, 100, &b) == 0 && b && b != a && g_live == live0 + 2);
  CHECK(scratch->get(nullptr, 100, &c) == 0 && c && c != a && c != b && g_live == live0 + 3);
  g_dev = 1;
  CHECK(scratch->get(&s1, 100, &d) == 0 && d && d != a && d != b && d != c && g_live == live0 + 4);
  memset(a, 1, 100); memset(b, 2, 100); memset(c, 3, 100); memset(d, 4, 100);
  CHECK(((char*)a)[99] == 1 && ((char*)b)[0] == 2 && ((char*)c)[50] == 3 && ((char*)d)[99] == 4);
  // the same key: the same array while the asked size fits, whatever happened on other keys meanwhile
  g_dev = 0;
  CHECK(scratch->get(&s1, 100, &p) == 0 && p == a);
  CHECK(scratch->get(&s1, 1, &p) == 0 && p == a);
  CHECK(scratch->get(&s1, 0, &p) == 0 && p == a && g_live == live0 + 4);
  // growth replaces the array (freed first: no more arrays than keys) and leaves the other keys' arrays alone
  CHECK(scratch->get(&s1, 5000, &p) == 0 && p && g_live == live0 + 4);
  memset(p, 5, 5000);
  CHECK(((char*)b)[99] == 2 && ((char*)d)[0] == 4);
  CHECK(scratch->get(&s1, 100, &a) == 0 && a == p);  // grow-only
  // a failed allocation: the call fails with a null pointer, the entry is left empty, and the next call works
  g_fail_alloc = true;
  CHECK(scratch->get(&s1, 100000, &p) == 1 && p == nullptr && g_live == live0 + 3);
  CHECK(scratch->get(&s2, 100, &p) == 0 && p == b);  // another key is untouched by it
  CHECK(scratch->get(&s1, 10, &p) == 0 && p && g_live == live0 + 4);
  memset(p, 6, 10);
  // an empty request on a new key: no array, no failure
  int s3 = 0;
  CHECK(scratch->get(&s3, 0, &p) == 0 && p == nullptr && g_live == live0 + 4);
  // two threads on different keys (their own device and stream), growing all the time: each sees only its own bytes
  bool ok[2] = {true, true};
  auto work = [&](int t) {
    g_dev = 2 + t;
    int st = 0;
    void* q = nullptr;
    for (size_t n = 1; n <= 4096 && ok[t]; n += 7) {
      ok[t] = scratch->get(&st, n, &q) == 0 && q;
      if (!ok[t]) break;
      memset(q, 10 + t, n);
      void* again = nullptr;
      ok[t] = scratch->get(&st, n / 2, &again) == 0 && again == q && ((char*)q)[n - 1] == 10 + t;
    }
  };
  std::thread t0(work, 0), t1(work, 1);
  t0.join();
  t1.join();
  CHECK(ok[0] && ok[1] && g_live == live0 + 6);
  g_dev = 0;
}

int main() {
  test_devbuf();
  test_cache();
  test_stream_scratch();
  if (g_bad) { fprintf(stderr, "%d checks failed\n", g_bad); return 1; }
  printf("devmem host checks passed\n");
  // the caches and the scratch are left alive on purpose, as in the library: their arrays are still reachable, which is no leak
  return 0;
}
