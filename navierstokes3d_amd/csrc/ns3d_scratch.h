// ns3d_scratch.h — the one owner type of the library's lazily grown device buffers (a context's ping-pong, hat, monitor, isosurface
// and voxelizer scratch; a rank's message, state and work buffers).  Internal; needs the HIP runtime API and ns3d_fail only.
#pragma once
#include <cstddef>

#include <hip/hip_runtime_api.h>

#include "../../include/ns3d.h"

int ns3d_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// Device memory an owner keeps between calls: grown on demand, never shrunk.  The destructor releases, so an owner has nothing to
// list; an owner that must free at a chosen point (its device current, its streams drained) calls release() or is destroyed there.
// Not copyable; movable (std::vector<MRank> grows), the moved-from object left empty.
struct ns3d_scratch {
    void *ptr = nullptr;
    size_t bytes = 0;
    ns3d_scratch() = default;
    ns3d_scratch(ns3d_scratch &&o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr; o.bytes = 0; }
    ns3d_scratch(const ns3d_scratch &) = delete;
    ns3d_scratch &operator=(const ns3d_scratch &) = delete;
    ~ns3d_scratch() { release(); }
    // bytes >= need: nothing.  Otherwise: if a buffer exists, drain() — whatever may still use it goes first; a non-zero return gives
    // up with the buffer kept — and free it; then allocate `need`.  A failed allocation leaves {nullptr, 0} and returns NS3D_ERR_HIP.
    template <class Drain>
    int reserve(size_t need, Drain drain)
    {
        if (bytes >= need) return NS3D_OK;
        if (ptr) {
            if (const int rc = drain()) return rc;
            release();
        }
        const hipError_t e = hipMalloc(&ptr, need);
        if (e != hipSuccess) {
            (void)hipGetLastError();        // reported through our status: leave no sticky error for the host framework
            ptr = nullptr;
            return ns3d_fail(NS3D_ERR_HIP, "hipMalloc(%zu bytes of scratch): %s", need, hipGetErrorString(e));
        }
        bytes = need;
        return NS3D_OK;
    }
    void release()                          // free if held; idempotent
    {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
    template <class T>
    T *as() const { return (T *)ptr; }
};
