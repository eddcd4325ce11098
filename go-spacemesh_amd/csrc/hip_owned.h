/* hip_owned.h — move-only owners of the four HIP resources the engine
 * holds: device memory, pinned host memory, streams and events.  Each frees
 * what it holds when it goes out of scope; an empty owner (never created,
 * creation failed, moved from) frees nothing.  Every creating call returns
 * hipError_t and first releases what the owner held before.
 *
 * The one rule of destruction order: a stream is synchronised before any
 * buffer or event queued on it is released.  ~Stream synchronises, and
 * locals and members die in reverse order of declaration, so declare a
 * Stream AFTER the buffers and events it uses.  An object whose streams
 * wait on each other's events synchronises all of them first in its own
 * destructor (PostInitSession). */
#ifndef POSTE_HIP_OWNED_H
#define POSTE_HIP_OWNED_H

#include <hip/hip_runtime.h>

#include <utility>

namespace hip_owned {

inline hipError_t free_device(void *p) { return hipFree(p); }
inline hipError_t free_pinned(void *p) { return hipHostFree(p); }
inline hipError_t free_event(hipEvent_t e) { return hipEventDestroy(e); }
inline hipError_t free_stream(hipStream_t s) {
  (void)hipStreamSynchronize(s);
  return hipStreamDestroy(s);
}

template <typename H, hipError_t (*Free)(H)> class Owned {
public:
  Owned() = default;
  Owned(const Owned &) = delete;
  Owned &operator=(const Owned &) = delete;
  Owned(Owned &&o) noexcept : h_(std::exchange(o.h_, H{})) {}
  Owned &operator=(Owned &&o) noexcept {
    if (this != &o) {
      reset();
      h_ = std::exchange(o.h_, H{});
    }
    return *this;
  }
  ~Owned() { reset(); }
  void reset() {
    if (h_) (void)Free(std::exchange(h_, H{}));
  }
  /* give the resource up, for one that lives as long as the process */
  H release() { return std::exchange(h_, H{}); }

protected:
  /* result of a creating call into h_: a failure leaves the owner empty */
  hipError_t made(hipError_t e) {
    if (e != hipSuccess) h_ = H{};
    return e;
  }
  H h_{};
};

/* sizes are in bytes, as hipMalloc and hipHostMalloc take them */
template <typename T> struct DevBuf : Owned<void *, free_device> {
  T *get() const { return static_cast<T *>(h_); }
  hipError_t alloc(size_t bytes) { return reset(), made(hipMalloc(&h_, bytes)); }
};

template <typename T> struct PinnedBuf : Owned<void *, free_pinned> {
  T *get() const { return static_cast<T *>(h_); }
  hipError_t alloc(size_t bytes) {
    return reset(), made(hipHostMalloc(&h_, bytes));
  }
};

struct Event : Owned<hipEvent_t, free_event> {
  hipEvent_t get() const { return h_; }
  hipError_t create(unsigned flags = hipEventDefault) {
    return reset(), made(hipEventCreateWithFlags(&h_, flags));
  }
};

struct Stream : Owned<hipStream_t, free_stream> {
  hipStream_t get() const { return h_; }
  hipError_t create() { return reset(), made(hipStreamCreate(&h_)); }
};

} // namespace hip_owned

#endif
