// zafx_devbuf.hpp -- the owners of plan-owned memory: DevBuf<T>, one device allocation, and PinnedBuf, one page-locked host allocation.
// Every device pointer of zafx_plan and PackedBand is one of these (zafx_internal.hpp): a table is a field and its upload, nothing else --
// the plan's destructor releases what the fields hold.
//
// Plain C++17: compiled by hipcc, by g++ (`make asan`) and, with -DZAFX_HOST_EMU, without the HIP headers (tests/host_emu/devbuf_emu.cpp,
// which defines the five allocator functions below over malloc / free and counts).
#pragma once
#include <cstddef>

#if defined(ZAFX_HOST_EMU)
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
#else
#include <hip/hip_runtime_api.h>
#endif

namespace zafx {

// The allocator under the owners (HIP: zafx_capi.cpp).  dev_alloc / dev_free and pinned_alloc / pinned_free keep the process-wide count of
// live plan-owned allocations (zafx_plan_live_allocations); a failed dev_alloc leaves *p null.
hipError_t dev_alloc(void** p, size_t bytes);
hipError_t dev_free(void* p);
hipError_t dev_copy_h2d(void* dst, const void* src, size_t bytes);   // synchronous
hipError_t pinned_alloc(void** p, size_t bytes);
hipError_t pinned_free(void* p);

template <class T, hipError_t (*ALLOC)(void**, size_t), hipError_t (*FREE)(void*)>
class OwnedBuf {   // move-only
public:
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf&& o) noexcept : p_(o.p_), bytes_(o.bytes_), owned_(o.owned_) { o.p_ = nullptr, o.bytes_ = 0, o.owned_ = true; }
    OwnedBuf& operator=(OwnedBuf&& o) noexcept {
        if (this != &o) {
            (void)reset();
            p_ = o.p_, bytes_ = o.bytes_, owned_ = o.owned_;
            o.p_ = nullptr, o.bytes_ = 0, o.owned_ = true;
        }
        return *this;
    }
    ~OwnedBuf() { (void)reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }   // a buffer is a kernel argument as it stands
    size_t bytes() const { return bytes_; }

    hipError_t reset() {
        if (!p_) return hipSuccess;
        void* const old = p_;
        const bool free_it = owned_;
        p_ = nullptr, bytes_ = 0, owned_ = true;
        return free_it ? FREE(old) : hipSuccess;
    }
    // A view of `o`'s allocation that owns nothing and frees nothing (run_mel_wide's STFT plan over the mel plan's tables); `o` outlives it.
    void borrow(const OwnedBuf& o) {
        (void)reset();
        p_ = o.p_, bytes_ = o.bytes_, owned_ = false;
    }
    // Grow-only: the allocation as it is when it holds `bytes`, else a new one of exactly `bytes` (the old one freed first; contents are not kept).
    hipError_t reserve(size_t bytes) {
        if (bytes <= bytes_) return hipSuccess;
        if (hipError_t e = reset(); e != hipSuccess) return e;
        void* fresh = nullptr;
        if (hipError_t e = ALLOC(&fresh, bytes); e != hipSuccess) return e;
        p_ = static_cast<T*>(fresh), bytes_ = bytes;
        return hipSuccess;
    }

protected:
    T* p_ = nullptr;
    size_t bytes_ = 0;
    bool owned_ = true;
};

// One device allocation.  upload() replaces the contents: the old allocation is freed FIRST -- the free waits for the kernels in flight, so
// a constant is never replaced under a kernel that still reads it --, zero bytes leave the buffer null, a failed allocation leaves it null.
template <class T>
class DevBuf : public OwnedBuf<T, dev_alloc, dev_free> {
public:
    hipError_t upload(const void* host, size_t bytes) {
        if (hipError_t e = this->reset(); e != hipSuccess) return e;
        if (hipError_t e = this->reserve(bytes); e != hipSuccess) return e;
        return bytes ? dev_copy_h2d(this->p_, host, bytes) : hipSuccess;
    }
};

// The page-locked twin (the staging copy of the ragged tables).
using PinnedBuf = OwnedBuf<void, pinned_alloc, pinned_free>;

}  // namespace zafx
