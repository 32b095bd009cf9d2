// Owners of the library's device (hipMalloc) and page-locked host (hipHostMalloc) memory.  Every allocation the library keeps is
// one of these, the matrices that contexts share (npbnn_share_data: FeatureStore, npbnn_ctx.hip.h) included; the only other calls of
// the allocator are npbnn_pinned_alloc / npbnn_pinned_free (memory handed to the caller).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "npbnn_hip.h"

namespace npbnn_api {

int fail(npbnn_ctx* ctx, int code, const char* fmt, ...);

enum class Mem { kDevice, kPinned };

// One allocation of T: move-only, freed by its destructor.  It converts to T* so that launches and copies read as they would with
// the raw pointer; what it holds is freed by reset() or the destructor and by nothing else.
template <typename T, Mem kKind>
class Buffer {
  public:
    Buffer() = default;
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    Buffer(Buffer&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    Buffer& operator=(Buffer&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_; n_ = o.n_;
            o.p_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    ~Buffer() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    size_t size() const { return n_; }      // capacity, in elements of T

    void reset() {
        if (p_) (void)(kKind == Mem::kDevice ? hipFree(p_) : hipHostFree(p_));
        p_ = nullptr;
        n_ = 0;
    }

    // Room for at least n elements.  Short of that, the old allocation is freed first (peak memory: the new one alone) and
    // alloc_n >= n elements (0: n) are allocated; contents are discarded, never copied.  On failure the buffer is left empty, so the
    // next call allocates again, and the error goes through fail(ctx, NPBNN_E_HIP, ...).  *grown: whether it reallocated.
    int reserve(npbnn_ctx* ctx, size_t n, size_t alloc_n = 0, bool* grown = nullptr, const char* file = __builtin_FILE(),
                int line = __builtin_LINE()) {
        if (grown) *grown = false;
        if (n <= n_) return NPBNN_OK;
        reset();
        if (alloc_n < n) alloc_n = n;
        void* p = nullptr;
        const hipError_t e = kKind == Mem::kDevice ? hipMalloc(&p, alloc_n * sizeof(T)) : hipHostMalloc(&p, alloc_n * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess)
            return fail(ctx, NPBNN_E_HIP, "%s(%zu bytes) failed: %s (%s:%d)", kKind == Mem::kDevice ? "hipMalloc" : "hipHostMalloc",
                        alloc_n * sizeof(T), hipGetErrorString(e), file, line);
        p_ = static_cast<T*>(p);
        n_ = alloc_n;
        if (grown) *grown = true;
        return NPBNN_OK;
    }

  private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

template <typename T>
using DevBuf = Buffer<T, Mem::kDevice>;
template <typename T>
using PinnedBuf = Buffer<T, Mem::kPinned>;

}  // namespace npbnn_api
