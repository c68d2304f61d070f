// snarkjs_amd/csrc/fflonk_verify.hip — batch FFLONK verification (src/fflonk_verify.js:28-137) on the device, gfx950, BN254.
//
// Per verifying key (zkmi_fflonk_vk_load): one lane brings C0 to Montgomery form with its on-curve flag and its transcript bytes, checks X_2 on
// its curve, builds the line tables of X_2 and of the G2 generator and the Fr constants (k1 k2 wr, w = Fr.w[power], 1/n, the powers of w8 w4 w3)
// — fflonk_verify.cuh fflonk_vk_prepare. Per proof (one lane each): fflonk_verify_one — input checks, the Keccak-256 transcript, the Fr part
// with one batched inversion, A1 by one five-base Straus sum, the two-table Miller loop, the final exponentiation.
//
// BLS12-381 is refused: the reference's fflonk.setup / fflonk.prove do not work on it, so there is no verdict to hold one to.
//
// Isolation: this verifier has a stream, device buffers, a key map and a mutex of its own — it shares nothing with the Groth16 and PLONK
// verifiers (whose contexts are private to their units), selects no pipeline slot and touches no MSM job slot or prover buffer. The coupling
// they document holds here too: growing a buffer or releasing a key calls hipFree, which waits for the whole device.
#include <mutex>
#include <map>
#include <stddef.h>
#include <string.h>
#include "zkmi_common.hpp"
#include "pairing_host.hpp"
#include "fflonk_verify.cuh"

namespace zkmi {
namespace {

constexpr int FFLONK_VERIFY_BLOCK = 64;

template <class C> __global__ void __launch_bounds__(64) k_fflonk_vk_prepare(const uint32_t* in, uint32_t power, uint32_t n_public, const PairingConsts<C>* K, FflonkVk<C>* vk,
                                                                             Line<C>* tabs) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    constexpr int N = C::N;
    // in: C0 (3 Fq), X_2 (3 Fq2), k1 k2 w3 w4 w8 wr, omega (8 words each)
    fflonk_vk_prepare(in, in + 3 * N, in + 9 * N, in + 9 * N + 48, power, n_public, K, vk, tabs, tabs + miller_lines<C>());
}

template <class C> __global__ void __launch_bounds__(FFLONK_VERIFY_BLOCK) k_fflonk_verify(const uint32_t* recs, const uint32_t* pubs, uint64_t n, FflonkVkView<C> V,
                                                                                         const PairingConsts<C>* K, int8_t* out, FflonkTrace<C>* tr) {
    const uint64_t i = (uint64_t)blockIdx.x * FFLONK_VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = (int8_t)fflonk_verify_one(recs + i * fflonk_record_words<C>(), pubs + i * 8 * V.vk->n_public, V, K, tr);
}

struct FflonkVkEntry {
    int curve = 0;
    uint32_t n_public = 0;
    void *d_vk = nullptr, *d_tabs = nullptr;
};
struct FflonkVerifyCtx {
    std::mutex mu;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;               // around the last verify kernel
    bool timed = false;
    void* d_consts = nullptr;
    DevBuf in_a, in_b, out, trace;
    std::map<uint64_t, FflonkVkEntry> keys;
    uint64_t next = 1;
};
FflonkVerifyCtx& fctx() {
    static FflonkVerifyCtx v;
    return v;
}

int grow(DevBuf& b, size_t bytes) {
    if (b.cap >= bytes) return ZKMI_OK;
    if (b.p) ZK_HIP(hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    ZK_HIP(hipMalloc(&b.p, bytes < 256 ? 256 : bytes));
    b.cap = bytes < 256 ? 256 : bytes;
    return ZKMI_OK;
}

template <class C> int consts_dev(const PairingConsts<C>** out) {
    FflonkVerifyCtx& v = fctx();
    if (!v.d_consts) {
        PairingConsts<C> K;
        pairing_consts_host(K);
        ZK_HIP(hipMalloc(&v.d_consts, sizeof K));
        ZK_HIP(hipMemcpyAsync(v.d_consts, &K, sizeof K, hipMemcpyHostToDevice, v.stream));
        ZK_HIP(hipStreamSynchronize(v.stream));
    }
    *out = (const PairingConsts<C>*)v.d_consts;
    return ZKMI_OK;
}

int begin() {
    ZK_TRY(require_ctx());
    FflonkVerifyCtx& v = fctx();
    if (!v.stream) {
        ZK_HIP(hipStreamCreateWithFlags(&v.stream, hipStreamNonBlocking));
        ZK_HIP(hipEventCreate(&v.ev0));
        ZK_HIP(hipEventCreate(&v.ev1));
    }
    return ZKMI_OK;
}

template <class C> int vk_build(FflonkVkEntry& e, const std::vector<uint8_t>& in, uint32_t power, uint32_t n_public, uint32_t* bad) {
    FflonkVerifyCtx& v = fctx();
    const PairingConsts<C>* K;
    ZK_TRY(consts_dev<C>(&K));
    ZK_HIP(hipMalloc(&e.d_vk, sizeof(FflonkVk<C>)));
    ZK_HIP(hipMalloc(&e.d_tabs, 2 * miller_lines<C>() * sizeof(Line<C>)));
    ZK_TRY(grow(v.in_a, in.size()));
    ZK_HIP(hipMemcpyAsync(v.in_a.p, in.data(), in.size(), hipMemcpyHostToDevice, v.stream));
    hipLaunchKernelGGL(k_fflonk_vk_prepare<C>, dim3(1), dim3(64), 0, v.stream, (const uint32_t*)v.in_a.p, power, n_public, K, (FflonkVk<C>*)e.d_vk, (Line<C>*)e.d_tabs);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(bad, (const uint8_t*)e.d_vk + offsetof(FflonkVk<C>, bad), 4, hipMemcpyDeviceToHost, v.stream));
    ZK_HIP(hipStreamSynchronize(v.stream));
    return ZKMI_OK;
}

template <class C> int vk_load(const uint8_t* c0, const uint8_t* x2, const uint8_t* consts, uint32_t power, uint32_t n_public, uint64_t* handle) {
    FflonkVerifyCtx& v = fctx();
    constexpr int N = C::N;
    const size_t f1 = 3 * 4 * N, f2 = 6 * 4 * N;
    std::vector<uint8_t> in(f1 + f2 + 192 + 32);
    memcpy(in.data(), c0, f1);
    memcpy(in.data() + f1, x2, f2);
    memcpy(in.data() + f1 + f2, consts, 192);
    ZK_TRY(fr_root(ZKMI_CURVE_BN128, power, in.data() + f1 + f2 + 192));          // Fr.w[power], Montgomery
    FflonkVkEntry e;
    e.curve = ZKMI_CURVE_BN128;
    e.n_public = n_public;
    uint32_t bad = 0;
    int rc = vk_build<C>(e, in, power, n_public, &bad);
    if (!rc && bad) rc = fail(ZKMI_ERR_INVALID, "fflonk_vk_load: X_2 is not on the curve");
    if (rc) {                                              // nothing of a failed load stays allocated
        (void)hipStreamSynchronize(v.stream);
        if (e.d_vk) (void)hipFree(e.d_vk);
        if (e.d_tabs) (void)hipFree(e.d_tabs);
        return rc;
    }
    *handle = v.next++;
    v.keys[*handle] = e;
    return ZKMI_OK;
}

template <class C> int verify_batch(const FflonkVkEntry& e, const uint8_t* proofs, const uint8_t* publics, size_t n, int8_t* verdicts, uint8_t* trace_out) {
    FflonkVerifyCtx& v = fctx();
    const PairingConsts<C>* K;
    ZK_TRY(consts_dev<C>(&K));
    const size_t rec = 4 * (size_t)fflonk_record_words<C>(), pub = (size_t)e.n_public * 32;
    ZK_TRY(grow(v.in_a, n * rec));
    ZK_TRY(grow(v.in_b, n * pub + 32));
    ZK_TRY(grow(v.out, n));
    if (trace_out) {
        ZK_TRY(grow(v.trace, sizeof(FflonkTrace<C>)));
        ZK_HIP(hipMemsetAsync(v.trace.p, 0, sizeof(FflonkTrace<C>), v.stream));
    }
    ZK_HIP(hipMemcpyAsync(v.in_a.p, proofs, n * rec, hipMemcpyHostToDevice, v.stream));
    if (pub) ZK_HIP(hipMemcpyAsync(v.in_b.p, publics, n * pub, hipMemcpyHostToDevice, v.stream));
    const Line<C>* tabs = (const Line<C>*)e.d_tabs;
    FflonkVkView<C> V{(const FflonkVk<C>*)e.d_vk, tabs, tabs + miller_lines<C>()};
    ZK_HIP(hipEventRecord(v.ev0, v.stream));
    hipLaunchKernelGGL(k_fflonk_verify<C>, dim3((unsigned)((n + FFLONK_VERIFY_BLOCK - 1) / FFLONK_VERIFY_BLOCK)), dim3(FFLONK_VERIFY_BLOCK), 0, v.stream,
                       (const uint32_t*)v.in_a.p, (const uint32_t*)v.in_b.p, (uint64_t)n, V, K, (int8_t*)v.out.p, trace_out ? (FflonkTrace<C>*)v.trace.p : nullptr);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipEventRecord(v.ev1, v.stream));
    v.timed = true;
    ZK_HIP(hipMemcpyAsync(verdicts, v.out.p, n, hipMemcpyDeviceToHost, v.stream));
    if (trace_out) ZK_HIP(hipMemcpyAsync(trace_out, v.trace.p, sizeof(FflonkTrace<C>), hipMemcpyDeviceToHost, v.stream));
    ZK_HIP(hipStreamSynchronize(v.stream));
    return ZKMI_OK;
}

int verify_entry(const char* who, uint64_t vk_handle, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, int8_t* verdicts, uint8_t* trace_out) {
    ZK_TRY(begin());
    auto it = fctx().keys.find(vk_handle);
    if (it == fctx().keys.end()) return fail(ZKMI_ERR_INVALID, std::string(who) + ": unknown verifying key");
    const FflonkVkEntry& e = it->second;
    if (n_signals != e.n_public) return fail(ZKMI_ERR_INVALID, "Number of public signals does not match with vk");
    if (n == 0) return ZKMI_OK;
    if (!proofs || !verdicts || (n_signals && !publics)) return fail(ZKMI_ERR_INVALID, std::string(who) + ": null argument");
    return verify_batch<Bn254Fq>(e, proofs, publics, n, verdicts, trace_out);
}

}  // namespace
}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zkmi_fflonk_vk_load(int curve, const uint8_t* c0_xyz, const uint8_t* x2_xyz, const uint8_t* consts, uint32_t power, uint32_t n_public, uint64_t* vk_handle) {
    std::lock_guard<std::mutex> g(fctx().mu);
    ZK_TRY(begin());
    if (!c0_xyz || !x2_xyz || !consts || !vk_handle) return fail(ZKMI_ERR_INVALID, "fflonk_vk_load: null argument");
    if (curve == ZKMI_CURVE_BLS12381) return fail(ZKMI_ERR_INVALID, "fflonk_vk_load: FFLONK verification serves BN254 only (the reference has no FFLONK on BLS12-381)");
    if (curve != ZKMI_CURVE_BN128) return fail(ZKMI_ERR_INVALID, "fflonk_vk_load: unknown curve");
    if (power > 28u) return fail(ZKMI_ERR_INVALID, "fflonk_vk_load: power beyond the field's two-adicity");
    return vk_load<Bn254Fq>(c0_xyz, x2_xyz, consts, power, n_public, vk_handle);
}

int zkmi_fflonk_verify_batch(uint64_t vk_handle, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, int8_t* verdicts) {
    std::lock_guard<std::mutex> g(fctx().mu);
    return verify_entry("fflonk_verify_batch", vk_handle, proofs, publics, n_signals, n, verdicts, nullptr);
}

int zkmi_fflonk_verify_trace_dev(uint64_t vk_handle, const uint8_t* proof, const uint8_t* publics, uint32_t n_signals, uint8_t* out) {
    std::lock_guard<std::mutex> g(fctx().mu);
    if (!out) return fail(ZKMI_ERR_INVALID, "fflonk_verify_trace_dev: null argument");
    int8_t verdict = 0;
    return verify_entry("fflonk_verify_trace_dev", vk_handle, proof, publics, n_signals, 1, &verdict, out);
}

int zkmi_fflonk_vk_info(uint64_t vk_handle, int* curve, uint32_t* n_public) {
    std::lock_guard<std::mutex> g(fctx().mu);
    auto it = fctx().keys.find(vk_handle);
    if (it == fctx().keys.end()) return fail(ZKMI_ERR_INVALID, "fflonk_vk_info: unknown verifying key");
    if (curve) *curve = it->second.curve;
    if (n_public) *n_public = it->second.n_public;
    return ZKMI_OK;
}

double zkmi_fflonk_verify_last_ms(void) {
    std::lock_guard<std::mutex> g(fctx().mu);
    FflonkVerifyCtx& v = fctx();
    float ms = 0;
    if (!v.timed || hipEventElapsedTime(&ms, v.ev0, v.ev1) != hipSuccess) return -1.0;
    return ms;
}

int zkmi_fflonk_vk_release(uint64_t vk_handle) {
    std::lock_guard<std::mutex> g(fctx().mu);
    ZK_TRY(begin());
    auto it = fctx().keys.find(vk_handle);
    if (it == fctx().keys.end()) return fail(ZKMI_ERR_INVALID, "fflonk_vk_release: unknown verifying key");
    ZK_HIP(hipFree(it->second.d_vk));
    ZK_HIP(hipFree(it->second.d_tabs));
    fctx().keys.erase(it);
    return ZKMI_OK;
}

}  // extern "C"
