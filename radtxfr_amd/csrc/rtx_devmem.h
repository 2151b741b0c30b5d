// Ownership of device memory ("Device memory"): an owned, grow-only device array, scratch per (device,
// stream) and a keyed cache of process-lifetime device tables. Host-only and free of HIP headers: everything goes through
// four functions that the library defines once (rtx_lines.hip) and that a host test may define over malloc.
#pragma once
#include <stddef.h>
#include <string.h>

#include <map>
#include <mutex>
#include <utility>
#include <vector>

int rtx_dev_alloc(void** p, size_t bytes);  // 0 ok; on failure *p = nullptr and the error text is set
void rtx_dev_free(void* p);                 // nullptr allowed; waits for the device, like hipFree
int rtx_dev_h2d(void* d, const void* h, size_t bytes);  // synchronous copy; 0 ok, else the error text is set
// index of the calling thread's current device; 0 ok, else the error text is set (hidden: the library's exported names stay
// what they were)
__attribute__((visibility("hidden"))) int rtx_dev_current(int* dev);

// Move-only owner of a device array of cap() elements. A failed reserve() or upload() leaves it empty: (nullptr, 0).
template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_; cap_ = o.cap_;
      o.p_ = nullptr; o.cap_ = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }

  T* get() const { return p_; }
  size_t cap() const { return cap_; }
  void reset() {
    rtx_dev_free(p_);
    p_ = nullptr; cap_ = 0;
  }
  // Grow-only, contents not kept. Growth frees first: the free waits for the device, so a kernel already enqueued on the
  // old array has finished before the array goes.
  int reserve(size_t n) {
    if (n <= cap_) return 0;
    reset();
    if (rtx_dev_alloc((void**)&p_, n * sizeof(T))) return 1;
    cap_ = n;
    return 0;
  }
  // reserve(n), then a synchronous copy of h[0, n): the source may be a caller's temporary.
  int upload(const T* h, size_t n) {
    if (reserve(n)) return 1;
    if (n && rtx_dev_h2d(p_, h, n * sizeof(T))) { reset(); return 1; }
    return 0;
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// Scratch of an entry point: grow-only device bytes per (current device, stream), the stream a hipStream_t passed as
// void*. Calls on one stream are ordered by it and may share bytes; calls on different streams (or devices) must not.
// get() hands out at least `bytes` bytes; the mutex covers the lookup and the reserve only. That is enough: map nodes do
// not move, and a call on another key only ever grows its own entry, so the pointer stays good until the next get() on
// the same key asks for more (growth frees first, and the free waits for the kernels enqueued on the old array).
// Every entry point keeps an object of its own: two of them can be live in one stream's call. One that lives as long as
// the process is made with `new` and never destroyed: no device call may run from a static destructor.
class StreamScratch {
 public:
  int get(void* stream, size_t bytes, void** out) {
    *out = nullptr;
    int dev = 0;
    if (rtx_dev_current(&dev)) return 1;
    std::lock_guard<std::mutex> lock(mu_);
    DevBuf<char>& b = buf_[std::make_pair(dev, stream)];
    if (b.reserve(bytes)) return 1;
    *out = b.get();
    return 0;
  }

 private:
  std::mutex mu_;
  std::map<std::pair<int, void*>, DevBuf<char>> buf_;
};

// Device tables that live as long as the process, keyed on (device index, a blob of bytes), at most max_entries of them
// (0: unbounded); a full cache forgets its oldest entry. get() hands out the table TOGETHER WITH THE HELD LOCK: the caller
// lets go of it only after it has enqueued the kernel that reads the table, so an eviction by another host thread (a free,
// which waits for the device) can only come after that launch. A cache object is made with `new` and never destroyed: no
// device call may run from a static destructor.
template <class T>
class DevTableCache {
 public:
  struct Hit {
    const T* d = nullptr;
    std::unique_lock<std::mutex> lock;
  };
  explicit DevTableCache(size_t max_entries) : max_(max_entries) {}

  // On a miss build(std::vector<T>& host) fills the table to upload and returns 0; a failed build or upload inserts nothing.
  template <class Build>
  int get(int dev, const void* key, size_t key_bytes, Build&& build, Hit* out) {
    std::unique_lock<std::mutex> lock(mu_);
    const Entry* hit = nullptr;
    for (const Entry& e : entries_)
      if (e.dev == dev && e.key.size() == key_bytes && (key_bytes == 0 || memcmp(e.key.data(), key, key_bytes) == 0)) { hit = &e; break; }
    if (!hit) {
      Entry e;
      std::vector<T> host;
      if (build(host) || e.d.upload(host.data(), host.size())) return 1;
      e.dev = dev;
      if (key_bytes) e.key.assign((const unsigned char*)key, (const unsigned char*)key + key_bytes);
      if (max_ && entries_.size() >= max_) entries_.erase(entries_.begin());
      entries_.push_back(std::move(e));
      hit = &entries_.back();
    }
    out->d = hit->d.get();
    out->lock = std::move(lock);
    return 0;
  }

 private:
  struct Entry {
    int dev = 0;
    std::vector<unsigned char> key;
    DevBuf<T> d;
  };
  std::mutex mu_;
  size_t max_;
  std::vector<Entry> entries_;
};
