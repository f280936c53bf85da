// lsd_devbuf.h -- device memory of the host side (lsd_ctx.h: the context owns it): the one owner of a hipMalloc allocation, and the one carver
// that lays typed regions out in such a buffer.  hipMalloc and hipFree are called here and nowhere else.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <utility>

namespace lsdhip {

// One device allocation of `capacity()` elements of T; freed when the owner goes away.  Move-only.  Every call reports the HIP status,
// for HIPCHK.
template <class T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); return *this; }   // (o frees what this held)
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { (void)resize(0); }

    T* get() const { return p_; }
    size_t capacity() const { return cap_; }

    // Exactly `count` elements, contents undefined: frees, then allocates (count == 0: frees only).  The caller has made sure that
    // nothing on the device still uses the old allocation.  After a failure the buffer is empty.
    hipError_t resize(size_t count) {
        cap_ = 0;
        if (p_) { hipError_t e = hipFree(p_); p_ = nullptr; if (e != hipSuccess) return e; }
        if (count == 0) return hipSuccess;
        hipError_t e = hipMalloc((void**)&p_, count * sizeof(T));
        if (e == hipSuccess) cap_ = count;
        return e;
    }

    // At least `count` elements, grow-only.  Nothing happens -- no allocation, no synchronisation -- while the capacity suffices; else the
    // device is drained first (kernels of earlier calls may still use the old allocation) and the capacity is 0 from then on until the
    // new allocation has succeeded.
    hipError_t reserve(size_t count) {
        if (count <= cap_) return hipSuccess;
        cap_ = 0;
        hipError_t e = hipDeviceSynchronize();
        return e != hipSuccess ? e : resize(count);
    }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

// Staging and workspace arenas: typed regions laid out one after the other in a byte buffer, each on its own 256-byte boundary (which
// covers the 16-byte accesses of the ingest and occupancy kernels); a region of no elements still gets an address of its own.
// The layout is a callable that names every region once, `k(pointer, element count)`; the pointer's type gives the element size.
class Carver {
public:
    explicit Carver(uint8_t* base) : at_(reinterpret_cast<uintptr_t>(base)) {}
    template <class T>
    void operator()(T*& region, size_t count) {
        region = reinterpret_cast<T*>(at_);
        const size_t bytes = count * sizeof(T);
        at_ += ((bytes ? bytes : 1) + kAlign - 1) & ~(kAlign - 1);
    }
    size_t bytes_from(uint8_t* base) const { return at_ - reinterpret_cast<uintptr_t>(base); }

private:
    static constexpr size_t kAlign = 256;
    uintptr_t at_;
};

// Runs `layout` once to measure, grows `buf` (DevBuf::reserve: nothing but the pointer arithmetic while it is large enough), then once
// more to hand the regions out.
template <class Layout>
hipError_t carve(DevBuf<uint8_t>& buf, Layout&& layout) {
    Carver measure(nullptr);
    layout(measure);
    hipError_t e = buf.reserve(measure.bytes_from(nullptr));
    if (e != hipSuccess) return e;
    Carver place(buf.get());
    layout(place);
    return hipSuccess;
}

}  // namespace lsdhip
