// Pinned staging of the grouped calls' descriptor tables (umlh_kernels_gauss.hip, umlh_kernels_align.hip): two buffers per device,
// each reused once the copy of its last use has finished (an event behind that copy), grown when a call needs more.  The source
// of the asynchronous upload therefore outlives it, and a call waits on the host only for a copy that is two calls old.  Every
// user owns one StageRings object: its calls do not wait on another user's copies.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <mutex>

struct StageRings {
    struct Ring {
        unsigned char* buf[2];
        size_t cap[2];
        hipEvent_t ev[2];
        bool used[2];
        int next;
        bool ready;
    };
    Ring dev[64];
    std::mutex mu;

    // dst[0, bytes) = what fill writes into a staging buffer, as one copy on st
    template <class Fill>
    int upload(void* dst, size_t bytes, hipStream_t st, Fill fill) {
        int d = 0;
        if (hipError_t e = hipGetDevice(&d)) return (int)e;
        std::lock_guard<std::mutex> lk(mu);
        Ring& S = dev[d & 63];
        if (!S.ready) {
            for (int i = 0; i < 2; ++i)
                if (hipError_t e = hipEventCreateWithFlags(&S.ev[i], hipEventDisableTiming)) return (int)e;
            S.ready = true;
        }
        const int i = S.next;
        S.next ^= 1;
        if (S.used[i])
            if (hipError_t e = hipEventSynchronize(S.ev[i])) return (int)e;
        if (S.cap[i] < bytes) {
            if (S.buf[i]) (void)hipHostFree(S.buf[i]);
            S.buf[i] = nullptr;
            S.cap[i] = 0;
            const size_t cap = (bytes + 65535) / 65536 * 65536;
            if (hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&S.buf[i]), cap, hipHostMallocDefault)) return (int)e;
            S.cap[i] = cap;
        }
        fill(S.buf[i]);
        if (hipError_t e = hipMemcpyAsync(dst, S.buf[i], bytes, hipMemcpyHostToDevice, st)) return (int)e;
        S.used[i] = true;
        return (int)hipEventRecord(S.ev[i], st);
    }
};
