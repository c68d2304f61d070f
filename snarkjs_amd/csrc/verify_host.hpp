// snarkjs_amd/csrc/verify_host.hpp — the host scaffold of the batch verifiers (groth16_verify.hip, plonk_verify.hip, fflonk_verify.hip).
//
// Isolation: every verifier instantiates VerifyCtx<its key entry> once, as a function-local static of its own translation unit, and so has a
// stream, two events, device buffers, a key map, handles (from 1) and a mutex of its own. It shares nothing with the other verifiers, never
// selects a pipeline slot and never touches the MSM job slots or a prover buffer, so a verify batch enqueued while a proof is in flight leaves
// that proof alone. Calls into one verifier are serialised by its mutex. One coupling remains: growing a buffer, and releasing a key, call
// hipFree, which waits for the whole device — a verify call that has to grow its buffers stalls until the kernels of an in-flight proof have
// finished (results are unaffected; buffers only grow).
//
// A key entry has `int curve`, `uint32_t n_public` and `void* blocks[N]`, the device blocks it owns: release() and drop() free them here.
#pragma once
#include <mutex>
#include <map>
#include <string>
#include "zkmi_common.hpp"
#include "pairing_host.hpp"

namespace zkmi {

constexpr int VERIFY_BLOCK = 64;                           // lanes per block of every per-proof kernel
inline unsigned verify_grid(size_t n) { return (unsigned)((n + VERIFY_BLOCK - 1) / VERIFY_BLOCK); }

inline int grow(DevBuf& b, size_t bytes) {
    if (b.cap >= bytes) return ZKMI_OK;
    if (b.p) ZK_HIP(hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    ZK_HIP(hipMalloc(&b.p, bytes < 256 ? 256 : bytes));
    b.cap = bytes < 256 ? 256 : bytes;
    return ZKMI_OK;
}

template <class Entry> struct VerifyCtx {
    std::mutex mu;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;               // around the last verify kernel
    bool timed = false;
    void* d_consts[2] = {nullptr, nullptr};                // PairingConsts per curve
    DevBuf in_a, in_b, out, trace;
    std::map<uint64_t, Entry> keys;
    uint64_t next = 1;

    int begin() {
        ZK_TRY(require_ctx());
        if (!stream) {
            ZK_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
            ZK_HIP(hipEventCreate(&ev0));
            ZK_HIP(hipEventCreate(&ev1));
        }
        return ZKMI_OK;
    }

    template <class C> int consts(const PairingConsts<C>** out_k) {
        const int ci = C::N == 8 ? 0 : 1;
        if (!d_consts[ci]) {
            PairingConsts<C> K;
            pairing_consts_host(K);
            ZK_HIP(hipMalloc(&d_consts[ci], sizeof K));
            ZK_HIP(hipMemcpyAsync(d_consts[ci], &K, sizeof K, hipMemcpyHostToDevice, stream));
            ZK_HIP(hipStreamSynchronize(stream));
        }
        *out_k = (const PairingConsts<C>*)d_consts[ci];
        return ZKMI_OK;
    }

    // null (and the error set) for a handle that names no key
    Entry* find(uint64_t handle, const char* who) {
        auto it = keys.find(handle);
        if (it != keys.end()) return &it->second;
        fail(ZKMI_ERR_INVALID, std::string(who) + ": unknown verifying key");
        return nullptr;
    }

    uint64_t add(const Entry& e) {
        keys[next] = e;
        return next++;
    }

    // nothing of a failed load stays allocated; returns rc
    int drop(Entry& e, int rc) {
        (void)hipStreamSynchronize(stream);
        for (void* b : e.blocks)
            if (b) (void)hipFree(b);
        return rc;
    }

    double last_ms() {
        float ms = 0;
        if (!timed || hipEventElapsedTime(&ms, ev0, ev1) != hipSuccess) return -1.0;
        return ms;
    }

    int info(uint64_t handle, const char* who, int* curve, uint32_t* n_public) {
        const Entry* e = find(handle, who);
        if (!e) return ZKMI_ERR_INVALID;
        if (curve) *curve = e->curve;
        if (n_public) *n_public = e->n_public;
        return ZKMI_OK;
    }

    int release(uint64_t handle, const char* who) {
        ZK_TRY(begin());
        Entry* e = find(handle, who);
        if (!e) return ZKMI_ERR_INVALID;
        for (void* b : e->blocks) ZK_HIP(hipFree(b));
        keys.erase(handle);
        return ZKMI_OK;
    }

    // One batch: a (a_bytes) to in_a and b (b_bytes, may be 0) to in_b, launch() on the stream between ev0 and ev1 when `time` is set, out_bytes
    // of `out` back to host_out and, where trace_out is given, the zeroed trace_bytes block the kernel wrote; returns after the stream is idle.
    template <class Launch>
    int run_batch(const void* a, size_t a_bytes, const void* b, size_t b_bytes, void* host_out, size_t out_bytes, void* trace_out, size_t trace_bytes, bool time,
                  Launch launch) {
        ZK_TRY(grow(in_a, a_bytes));
        ZK_TRY(grow(in_b, b_bytes + 32));
        ZK_TRY(grow(out, out_bytes));
        if (trace_out) {
            ZK_TRY(grow(trace, trace_bytes));
            ZK_HIP(hipMemsetAsync(trace.p, 0, trace_bytes, stream));
        }
        ZK_HIP(hipMemcpyAsync(in_a.p, a, a_bytes, hipMemcpyHostToDevice, stream));
        if (b_bytes) ZK_HIP(hipMemcpyAsync(in_b.p, b, b_bytes, hipMemcpyHostToDevice, stream));
        if (time) ZK_HIP(hipEventRecord(ev0, stream));
        launch();
        ZK_HIP(hipGetLastError());
        if (time) {
            ZK_HIP(hipEventRecord(ev1, stream));
            timed = true;
        }
        ZK_HIP(hipMemcpyAsync(host_out, out.p, out_bytes, hipMemcpyDeviceToHost, stream));
        if (trace_out) ZK_HIP(hipMemcpyAsync(trace_out, trace.p, trace_bytes, hipMemcpyDeviceToHost, stream));
        ZK_HIP(hipStreamSynchronize(stream));
        return ZKMI_OK;
    }
};

}  // namespace zkmi
