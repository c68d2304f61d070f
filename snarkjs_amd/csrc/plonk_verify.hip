// snarkjs_amd/csrc/plonk_verify.hip — batch PLONK verification (src/plonk_verify.js:29-123) on the device, gfx950.
//
// Per verifying key (zkmi_plonk_vk_load): one lane brings the eight key points to Montgomery form, checks them and X_2 on their curves, builds
// the line tables of X_2 and of the G2 generator and the Fr constants (w = Fr.w[power], 1/n, k1, k2) — plonk_verify.cuh plonk_vk_prepare.
// Per proof (one lane each): plonk_verify_one — input checks, the Keccak-256 transcript, the Fr part, B1 by one 18-base Straus sum, A1, the
// two-table Miller loop, the final exponentiation.
//
// Isolation: this verifier has a stream, device buffers, a key map and a mutex of its own — it shares nothing with the Groth16 verifier (whose
// context is private to groth16_verify.hip), selects no pipeline slot and touches no MSM job slot or prover buffer. The coupling the Groth16
// verifier documents holds here too: growing a buffer or releasing a key calls hipFree, which waits for the whole device.
#include <mutex>
#include <map>
#include <stddef.h>
#include <string.h>
#include "zkmi_common.hpp"
#include "pairing_host.hpp"
#include "plonk_verify.cuh"

namespace zkmi {
namespace {

constexpr int PLONK_VERIFY_BLOCK = 64;

template <class C> __global__ void __launch_bounds__(64) k_plonk_vk_prepare(const uint32_t* in, uint32_t power, uint32_t n_public, const PairingConsts<C>* K, PlonkVk<C>* vk,
                                                                             Line<C>* tabs) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    constexpr int N = C::N;
    // in: eight G1 points (3 Fq each), X_2 (3 Fq2), k1, k2, omega (8 words each)
    plonk_vk_prepare(in, in + 24 * N, in + 30 * N, in + 30 * N + 8, in + 30 * N + 16, power, n_public, K, vk, tabs, tabs + miller_lines<C>());
}

template <class C> __global__ void __launch_bounds__(PLONK_VERIFY_BLOCK) k_plonk_verify(const uint32_t* recs, const uint32_t* pubs, uint64_t n, PlonkVkView<C> V,
                                                                                         const PairingConsts<C>* K, int8_t* out, PlonkTrace<C>* tr) {
    const uint64_t i = (uint64_t)blockIdx.x * PLONK_VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = (int8_t)plonk_verify_one(recs + i * plonk_record_words<C>(), pubs + i * 8 * V.vk->n_public, V, K, tr);
}

struct PlonkVkEntry {
    int curve = 0;
    uint32_t n_public = 0;
    void *d_vk = nullptr, *d_tabs = nullptr;
};
struct PlonkVerifyCtx {
    std::mutex mu;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;               // around the last verify kernel
    bool timed = false;
    void* d_consts[2] = {nullptr, nullptr};
    DevBuf in_a, in_b, out, trace;
    std::map<uint64_t, PlonkVkEntry> keys;
    uint64_t next = 1;
};
PlonkVerifyCtx& pctx() {
    static PlonkVerifyCtx v;
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
    PlonkVerifyCtx& v = pctx();
    const int ci = C::N == 8 ? 0 : 1;
    if (!v.d_consts[ci]) {
        PairingConsts<C> K;
        pairing_consts_host(K);
        ZK_HIP(hipMalloc(&v.d_consts[ci], sizeof K));
        ZK_HIP(hipMemcpyAsync(v.d_consts[ci], &K, sizeof K, hipMemcpyHostToDevice, v.stream));
        ZK_HIP(hipStreamSynchronize(v.stream));
    }
    *out = (const PairingConsts<C>*)v.d_consts[ci];
    return ZKMI_OK;
}

int begin() {
    ZK_TRY(require_ctx());
    PlonkVerifyCtx& v = pctx();
    if (!v.stream) {
        ZK_HIP(hipStreamCreateWithFlags(&v.stream, hipStreamNonBlocking));
        ZK_HIP(hipEventCreate(&v.ev0));
        ZK_HIP(hipEventCreate(&v.ev1));
    }
    return ZKMI_OK;
}

template <class C> int vk_build(PlonkVkEntry& e, const std::vector<uint8_t>& in, uint32_t power, uint32_t n_public, uint32_t* bad) {
    PlonkVerifyCtx& v = pctx();
    const PairingConsts<C>* K;
    ZK_TRY(consts_dev<C>(&K));
    ZK_HIP(hipMalloc(&e.d_vk, sizeof(PlonkVk<C>)));
    ZK_HIP(hipMalloc(&e.d_tabs, 2 * miller_lines<C>() * sizeof(Line<C>)));
    ZK_TRY(grow(v.in_a, in.size()));
    ZK_HIP(hipMemcpyAsync(v.in_a.p, in.data(), in.size(), hipMemcpyHostToDevice, v.stream));
    hipLaunchKernelGGL(k_plonk_vk_prepare<C>, dim3(1), dim3(64), 0, v.stream, (const uint32_t*)v.in_a.p, power, n_public, K, (PlonkVk<C>*)e.d_vk, (Line<C>*)e.d_tabs);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(bad, (const uint8_t*)e.d_vk + offsetof(PlonkVk<C>, bad), 4, hipMemcpyDeviceToHost, v.stream));
    ZK_HIP(hipStreamSynchronize(v.stream));
    return ZKMI_OK;
}

template <class C> int vk_load(const uint8_t* g1, const uint8_t* x2, const uint8_t* k1, const uint8_t* k2, uint32_t power, uint32_t n_public, uint64_t* handle) {
    PlonkVerifyCtx& v = pctx();
    constexpr int N = C::N;
    const int curve = N == 8 ? ZKMI_CURVE_BN128 : ZKMI_CURVE_BLS12381;
    const size_t f1 = 3 * 4 * N, f2 = 6 * 4 * N;
    std::vector<uint8_t> in(8 * f1 + f2 + 96);
    memcpy(in.data(), g1, 8 * f1);
    memcpy(in.data() + 8 * f1, x2, f2);
    memcpy(in.data() + 8 * f1 + f2, k1, 32);
    memcpy(in.data() + 8 * f1 + f2 + 32, k2, 32);
    ZK_TRY(fr_root(curve, power, in.data() + 8 * f1 + f2 + 64));          // Fr.w[power], Montgomery
    PlonkVkEntry e;
    e.curve = curve;
    e.n_public = n_public;
    uint32_t bad = 0;
    int rc = vk_build<C>(e, in, power, n_public, &bad);
    if (!rc && bad) rc = fail(ZKMI_ERR_INVALID, "plonk_vk_load: a key point is not on the curve");
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

template <class C> int verify_batch(const PlonkVkEntry& e, const uint8_t* proofs, const uint8_t* publics, size_t n, int8_t* verdicts, uint8_t* trace_out) {
    PlonkVerifyCtx& v = pctx();
    const PairingConsts<C>* K;
    ZK_TRY(consts_dev<C>(&K));
    const size_t rec = 4 * (size_t)plonk_record_words<C>(), pub = (size_t)e.n_public * 32;
    ZK_TRY(grow(v.in_a, n * rec));
    ZK_TRY(grow(v.in_b, n * pub + 32));
    ZK_TRY(grow(v.out, n));
    if (trace_out) {
        ZK_TRY(grow(v.trace, sizeof(PlonkTrace<C>)));
        ZK_HIP(hipMemsetAsync(v.trace.p, 0, sizeof(PlonkTrace<C>), v.stream));
    }
    ZK_HIP(hipMemcpyAsync(v.in_a.p, proofs, n * rec, hipMemcpyHostToDevice, v.stream));
    if (pub) ZK_HIP(hipMemcpyAsync(v.in_b.p, publics, n * pub, hipMemcpyHostToDevice, v.stream));
    const Line<C>* tabs = (const Line<C>*)e.d_tabs;
    PlonkVkView<C> V{(const PlonkVk<C>*)e.d_vk, tabs, tabs + miller_lines<C>()};
    ZK_HIP(hipEventRecord(v.ev0, v.stream));
    hipLaunchKernelGGL(k_plonk_verify<C>, dim3((unsigned)((n + PLONK_VERIFY_BLOCK - 1) / PLONK_VERIFY_BLOCK)), dim3(PLONK_VERIFY_BLOCK), 0, v.stream,
                       (const uint32_t*)v.in_a.p, (const uint32_t*)v.in_b.p, (uint64_t)n, V, K, (int8_t*)v.out.p, trace_out ? (PlonkTrace<C>*)v.trace.p : nullptr);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipEventRecord(v.ev1, v.stream));
    v.timed = true;
    ZK_HIP(hipMemcpyAsync(verdicts, v.out.p, n, hipMemcpyDeviceToHost, v.stream));
    if (trace_out) ZK_HIP(hipMemcpyAsync(trace_out, v.trace.p, sizeof(PlonkTrace<C>), hipMemcpyDeviceToHost, v.stream));
    ZK_HIP(hipStreamSynchronize(v.stream));
    return ZKMI_OK;
}

int verify_entry(const char* who, uint64_t vk_handle, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, int8_t* verdicts, uint8_t* trace_out) {
    ZK_TRY(begin());
    auto it = pctx().keys.find(vk_handle);
    if (it == pctx().keys.end()) return fail(ZKMI_ERR_INVALID, std::string(who) + ": unknown verifying key");
    const PlonkVkEntry& e = it->second;
    if (n_signals != e.n_public) return fail(ZKMI_ERR_INVALID, "Invalid number of public inputs");
    if (n == 0) return ZKMI_OK;
    if (!proofs || !verdicts || (n_signals && !publics)) return fail(ZKMI_ERR_INVALID, std::string(who) + ": null argument");
    if (e.curve == ZKMI_CURVE_BN128) return verify_batch<Bn254Fq>(e, proofs, publics, n, verdicts, trace_out);
    return verify_batch<Bls12381Fq>(e, proofs, publics, n, verdicts, trace_out);
}

}  // namespace
}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zkmi_plonk_vk_load(int curve, const uint8_t* g1_points_xyz, const uint8_t* x2_xyz, const uint8_t* k1, const uint8_t* k2, uint32_t power, uint32_t n_public,
                       uint64_t* vk_handle) {
    std::lock_guard<std::mutex> g(pctx().mu);
    ZK_TRY(begin());
    if (!g1_points_xyz || !x2_xyz || !k1 || !k2 || !vk_handle) return fail(ZKMI_ERR_INVALID, "plonk_vk_load: null argument");
    if (curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) return fail(ZKMI_ERR_INVALID, "plonk_vk_load: unknown curve");
    if (power > (curve == ZKMI_CURVE_BN128 ? 28u : 32u)) return fail(ZKMI_ERR_INVALID, "plonk_vk_load: power beyond the field's two-adicity");
    if (curve == ZKMI_CURVE_BN128) return vk_load<Bn254Fq>(g1_points_xyz, x2_xyz, k1, k2, power, n_public, vk_handle);
    return vk_load<Bls12381Fq>(g1_points_xyz, x2_xyz, k1, k2, power, n_public, vk_handle);
}

int zkmi_plonk_verify_batch(uint64_t vk_handle, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, int8_t* verdicts) {
    std::lock_guard<std::mutex> g(pctx().mu);
    return verify_entry("plonk_verify_batch", vk_handle, proofs, publics, n_signals, n, verdicts, nullptr);
}

int zkmi_plonk_verify_trace_dev(uint64_t vk_handle, const uint8_t* proof, const uint8_t* publics, uint32_t n_signals, uint8_t* out) {
    std::lock_guard<std::mutex> g(pctx().mu);
    if (!out) return fail(ZKMI_ERR_INVALID, "plonk_verify_trace_dev: null argument");
    int8_t verdict = 0;
    return verify_entry("plonk_verify_trace_dev", vk_handle, proof, publics, n_signals, 1, &verdict, out);
}

int zkmi_plonk_vk_info(uint64_t vk_handle, int* curve, uint32_t* n_public) {
    std::lock_guard<std::mutex> g(pctx().mu);
    auto it = pctx().keys.find(vk_handle);
    if (it == pctx().keys.end()) return fail(ZKMI_ERR_INVALID, "plonk_vk_info: unknown verifying key");
    if (curve) *curve = it->second.curve;
    if (n_public) *n_public = it->second.n_public;
    return ZKMI_OK;
}

double zkmi_plonk_verify_last_ms(void) {
    std::lock_guard<std::mutex> g(pctx().mu);
    PlonkVerifyCtx& v = pctx();
    float ms = 0;
    if (!v.timed || hipEventElapsedTime(&ms, v.ev0, v.ev1) != hipSuccess) return -1.0;
    return ms;
}

int zkmi_plonk_vk_release(uint64_t vk_handle) {
    std::lock_guard<std::mutex> g(pctx().mu);
    ZK_TRY(begin());
    auto it = pctx().keys.find(vk_handle);
    if (it == pctx().keys.end()) return fail(ZKMI_ERR_INVALID, "plonk_vk_release: unknown verifying key");
    ZK_HIP(hipFree(it->second.d_vk));
    ZK_HIP(hipFree(it->second.d_tabs));
    pctx().keys.erase(it);
    return ZKMI_OK;
}

}  // extern "C"
