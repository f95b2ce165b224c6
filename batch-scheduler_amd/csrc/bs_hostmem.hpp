// bs_hostmem.hpp — the owner types of everything bs_ctx holds from the HIP runtime (host code only: no kernel includes this).
// Each frees what it owns in its destructor, so `delete ctx` releases a context at any point of its life.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace bs {

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    size_t want = std::max<size_t>(bytes, 256);
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// A stream or an event: move-only, reads as the handle it owns.
template <typename H, hipError_t (*Destroy)(H)>
struct Owned {
  H h = nullptr;
  Owned() = default;
  Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
  Owned& operator=(Owned&& o) noexcept { std::swap(h, o.h); return *this; }
  ~Owned() { if (h) (void)Destroy(h); }
  operator H() const { return h; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;

// How the host learns that the device is through with a pinned buffer it handed over (PinnedBuf::mark_busy): from an event recorded
// behind the work, by waiting for the stream the work went to, or not at all (the owner's protocol orders the accesses).
enum class PinWait { None, Event, Stream };

// Pinned host memory.  `cap` is in bytes; the growth rule is the caller's (reserve's `want`).
template <typename T = uint8_t>
struct PinnedBuf {
  T* p = nullptr;
  size_t cap = 0;
  bool busy = false;             // the device may still be reading the buffer; whoever sees the stream idle may clear it
  const PinWait how;
  const unsigned flags;          // of hipHostMalloc
  Event ev;                      // PinWait::Event: created by the first mark_busy
  hipStream_t on = nullptr;      // PinWait::Stream: where the last mark_busy's work went
  explicit PinnedBuf(PinWait how_ = PinWait::None, unsigned flags_ = hipHostMallocDefault) : how(how_), flags(flags_) {}
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
  hipError_t wait() {
    hipError_t e = hipSuccess;
    if (busy && how == PinWait::Event) e = hipEventSynchronize(ev);
    if (busy && how == PinWait::Stream) e = hipStreamSynchronize(on);
    if (e == hipSuccess) busy = false;
    return e;
  }
  // waits until the buffer is the host's again, then makes it hold `bytes` (a buffer that has to grow is allocated with `want` bytes)
  hipError_t reserve(size_t bytes, size_t want) {
    hipError_t e = wait();
    if (e != hipSuccess || bytes <= cap) return e;
    if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
    e = hipHostMalloc(reinterpret_cast<void**>(&p), want, flags);
    if (e == hipSuccess) cap = want;
    return e;
  }
  hipError_t reserve(size_t bytes) { return reserve(bytes, bytes); }
  // work that reads the buffer was just enqueued on `stream`
  hipError_t mark_busy(hipStream_t stream) {
    hipError_t e = hipSuccess;
    if (how == PinWait::Event) {
      if (!ev) e = hipEventCreateWithFlags(&ev.h, hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventRecord(ev, stream);
    }
    on = stream;
    if (e == hipSuccess) busy = true;
    return e;
  }
};

}  // namespace bs
