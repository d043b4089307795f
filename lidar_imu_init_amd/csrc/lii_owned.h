// The owners of the library's HIP resources.  A device buffer, a pinned buffer, a stream or an event that belongs to the handle
// (lii_context.h) or to the ingest ring (lii_ingest.hip) is a member of one of these four types: it is released when its owner goes,
// and nowhere else.  Move-only; each converts to the raw pointer / handle it holds, so launches and runtime calls take it as it is.
// alloc / grow / create return the runtime's status and sit inside HIPCHK (lii_launch.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

namespace lii {

// One allocation of n elements, released by Free.  size() is set only behind a successful allocation: pointer and capacity agree.
template <class T, hipError_t (*Free)(void*)>
class OwnedBuf {
 public:
  OwnedBuf() = default;
  OwnedBuf(OwnedBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  OwnedBuf& operator=(OwnedBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
    return *this;
  }
  ~OwnedBuf() { reset(); }
  void reset() {
    if (p_) (void)Free(p_);
    p_ = nullptr;
    n_ = 0;
  }
  size_t size() const { return n_; }  // elements; 0 when empty
  T* get() const { return p_; }
  operator T*() const { return p_; }
  T* operator->() const { return p_; }

 protected:
  hipError_t adopt(hipError_t e, void* p, size_t n) {
    if (e == hipSuccess) { p_ = static_cast<T*>(p); n_ = n; }
    return e;
  }
  T* p_ = nullptr;
  size_t n_ = 0;
};

template <class T>
class DevBuf : public OwnedBuf<T, hipFree> {
 public:
  hipError_t alloc(size_t n) {  // the buffer must be empty
    if (this->p_) return hipErrorInvalidValue;
    void* p = nullptr;
    return this->adopt(hipMalloc(&p, n * sizeof(T)), p, n);
  }
  // frees first, then allocates: the peak footprint of a growth is the larger of the two sizes, never their sum
  hipError_t grow(size_t n) { this->reset(); return alloc(n); }
  // room for n elements, the contents not kept: nothing when it is there, else max(n, twice the size) - scratch that creeps upwards
  // is released (hipFree waits for the device) a handful of times at most
  hipError_t at_least(size_t n) { return n <= this->n_ ? hipSuccess : grow(n > 2 * this->n_ ? n : 2 * this->n_); }
};

template <class T>
class PinnedBuf : public OwnedBuf<T, hipHostFree> {
 public:
  hipError_t alloc(size_t n, unsigned int flags) {  // hipHostMallocDefault / hipHostMallocMapped; the buffer must be empty
    if (this->p_) return hipErrorInvalidValue;
    void* p = nullptr;
    return this->adopt(hipHostMalloc(&p, n * sizeof(T), flags), p, n);
  }
  hipError_t at_least(size_t n, unsigned int flags) {  // as DevBuf::at_least
    if (n <= this->n_) return hipSuccess;
    const size_t want = n > 2 * this->n_ ? n : 2 * this->n_;
    this->reset();
    return alloc(want, flags);
  }
};

class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event& operator=(Event&&) = delete;
  ~Event() { if (e_) (void)hipEventDestroy(e_); }
  hipError_t create(unsigned int flags) { return e_ ? hipErrorInvalidValue : hipEventCreateWithFlags(&e_, flags); }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

// The destructor waits for the stream's work before it destroys the stream.
class Stream {
 public:
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() {
    if (s_) { (void)hipStreamSynchronize(s_); (void)hipStreamDestroy(s_); }
  }
  hipError_t create(unsigned int flags) { return s_ ? hipErrorInvalidValue : hipStreamCreateWithFlags(&s_, flags); }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};

}  // namespace lii
