// snarkjs_amd/csrc/groth16_verify.hip — batch Groth16 verification (src/groth16_verify.js:26-87) and the diagnostic pairing, gfx950.
//
// Per verifying key (zkmi_groth16_vk_load): the key's points go to Montgomery form and the line tables of beta, gamma, delta and the Miller
// value M(alpha, beta) are built once by one lane (pairing.cuh vk_prepare); every proof lane reads them. Per proof (one lane each):
// publics < r, pi_a / pi_b / pi_c on the curve (no subgroup check, as the reference), vk_x by interleaved double-and-add over the publics,
// the multi-Miller loop (pi_b walked, gamma and delta from their tables), times M(alpha, beta), the final exponentiation, == 1.
//
// Isolation from the provers: the verifier owns its stream, its device buffers and its key map; it never selects a pipeline slot and never
// touches the MSM job slots, so a verify batch enqueued while a proof is in flight leaves that proof alone. Calls are serialised by a mutex.
// One coupling remains: growing the verifier's buffers, and releasing a key, call hipFree, which waits for the whole device — a verify call
// that has to grow its buffers stalls until the kernels of an in-flight proof have finished (results are unaffected; buffers only grow).
#include <mutex>
#include <map>
#include <string.h>
#include "zkmi_common.hpp"
#include "pairing_host.hpp"

namespace zkmi {
namespace {

constexpr int VERIFY_BLOCK = 64;

template <class C> __global__ void __launch_bounds__(64) k_vk_prepare(const uint32_t* pts, uint32_t n_ic, const PairingConsts<C>* K, Fp<C>* ic,
                                                                       Line<C>* tabs, Fp12<C>* mab, uint32_t* flags) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    constexpr int N = C::N, NL = miller_lines<C>();
    // pts: alpha (3 Fq), beta, gamma, delta (3 Fq2 each), IC (3 Fq each)
    flags[0] = vk_prepare(pts, pts + 3 * N, pts + 9 * N, pts + 15 * N, pts + 21 * N, n_ic, K, ic, tabs, tabs + NL, tabs + 2 * NL, mab);
}

template <class C> __global__ void __launch_bounds__(VERIFY_BLOCK) k_g16_verify(const uint32_t* recs, const uint32_t* pubs, uint32_t n_sig, uint64_t n,
                                                                                 VkView<C> vk, const PairingConsts<C>* K, int8_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = (int8_t)groth16_verify_one(recs + i * 12 * C::N, pubs + i * 8 * n_sig, n_sig, vk, K);
}

template <class C> __global__ void __launch_bounds__(VERIFY_BLOCK) k_pairing(const uint32_t* g1, const uint32_t* g2, uint64_t n, const PairingConsts<C>* K,
                                                                              Fp<C>* out) {
    const uint64_t i = (uint64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    pairing_one(g1 + i * 3 * C::N, g2 + i * 6 * C::N, K, out + 12 * i);
}

struct VkEntry {
    int curve = 0;
    uint32_t n_public = 0, flags = 0;
    void *d_ic = nullptr, *d_tabs = nullptr, *d_mab = nullptr;
};
struct VerifyCtx {
    std::mutex mu;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;               // around the last verify / pairing kernel
    bool timed = false;
    void* d_consts[2] = {nullptr, nullptr};
    DevBuf in_a, in_b, out;
    std::map<uint64_t, VkEntry> keys;
    uint64_t next = 1;
};
VerifyCtx& vctx() {
    static VerifyCtx v;
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
    VerifyCtx& v = vctx();
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
    VerifyCtx& v = vctx();
    if (!v.stream) {
        ZK_HIP(hipStreamCreateWithFlags(&v.stream, hipStreamNonBlocking));
        ZK_HIP(hipEventCreate(&v.ev0));
        ZK_HIP(hipEventCreate(&v.ev1));
    }
    return ZKMI_OK;
}

template <class C> int vk_build(VkEntry& e, const std::vector<uint8_t>& pts, size_t n_ic, const PairingConsts<C>* K) {
    VerifyCtx& v = vctx();
    constexpr int NL = miller_lines<C>();
    ZK_HIP(hipMalloc(&e.d_ic, n_ic * 2 * sizeof(Fp<C>)));
    ZK_HIP(hipMalloc(&e.d_tabs, 3 * NL * sizeof(Line<C>)));
    ZK_HIP(hipMalloc(&e.d_mab, sizeof(Fp12<C>)));
    ZK_TRY(grow(v.in_a, pts.size()));
    ZK_TRY(grow(v.out, 16));
    ZK_HIP(hipMemcpyAsync(v.in_a.p, pts.data(), pts.size(), hipMemcpyHostToDevice, v.stream));
    hipLaunchKernelGGL(k_vk_prepare<C>, dim3(1), dim3(64), 0, v.stream, (const uint32_t*)v.in_a.p, (uint32_t)n_ic, K, (Fp<C>*)e.d_ic, (Line<C>*)e.d_tabs,
                       (Fp12<C>*)e.d_mab, (uint32_t*)v.out.p);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(&e.flags, v.out.p, 4, hipMemcpyDeviceToHost, v.stream));
    ZK_HIP(hipStreamSynchronize(v.stream));
    return ZKMI_OK;
}

template <class C> int vk_load(const uint8_t* alpha, const uint8_t* beta, const uint8_t* gamma, const uint8_t* delta, const uint8_t* ic, uint32_t n_public,
                               uint64_t* handle) {
    VerifyCtx& v = vctx();
    constexpr int N = C::N;
    const PairingConsts<C>* K;
    ZK_TRY(consts_dev<C>(&K));
    const size_t n_ic = (size_t)n_public + 1, f1 = 3 * 4 * N, f2 = 6 * 4 * N;
    std::vector<uint8_t> pts(f1 + 3 * f2 + n_ic * f1);
    memcpy(pts.data(), alpha, f1);
    memcpy(pts.data() + f1, beta, f2);
    memcpy(pts.data() + f1 + f2, gamma, f2);
    memcpy(pts.data() + f1 + 2 * f2, delta, f2);
    memcpy(pts.data() + f1 + 3 * f2, ic, n_ic * f1);
    VkEntry e;
    e.curve = N == 8 ? ZKMI_CURVE_BN128 : ZKMI_CURVE_BLS12381;
    e.n_public = n_public;
    const int rc = vk_build<C>(e, pts, n_ic, K);
    if (rc) {                                              // nothing of a failed load stays allocated
        (void)hipStreamSynchronize(v.stream);
        if (e.d_ic) (void)hipFree(e.d_ic);
        if (e.d_tabs) (void)hipFree(e.d_tabs);
        if (e.d_mab) (void)hipFree(e.d_mab);
        return rc;
    }
    *handle = v.next++;
    v.keys[*handle] = e;
    return ZKMI_OK;
}

template <class C> int verify_batch(const VkEntry& e, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, int8_t* verdicts) {
    VerifyCtx& v = vctx();
    constexpr int N = C::N, NL = miller_lines<C>();
    const PairingConsts<C>* K;
    ZK_TRY(consts_dev<C>(&K));
    const size_t rec = 12 * 4 * N, pub = (size_t)n_signals * 32;
    ZK_TRY(grow(v.in_a, n * rec));
    ZK_TRY(grow(v.in_b, n * pub));
    ZK_TRY(grow(v.out, n));
    ZK_HIP(hipMemcpyAsync(v.in_a.p, proofs, n * rec, hipMemcpyHostToDevice, v.stream));
    if (pub) ZK_HIP(hipMemcpyAsync(v.in_b.p, publics, n * pub, hipMemcpyHostToDevice, v.stream));
    const Line<C>* tabs = (const Line<C>*)e.d_tabs;
    VkView<C> vk{(const Fp<C>*)e.d_ic, e.n_public + 1, tabs + NL, tabs + 2 * NL, e.flags & 1u, (e.flags >> 1) & 1u, (const Fp12<C>*)e.d_mab};
    ZK_HIP(hipEventRecord(v.ev0, v.stream));
    hipLaunchKernelGGL(k_g16_verify<C>, dim3((unsigned)((n + VERIFY_BLOCK - 1) / VERIFY_BLOCK)), dim3(VERIFY_BLOCK), 0, v.stream, (const uint32_t*)v.in_a.p,
                       (const uint32_t*)v.in_b.p, n_signals, (uint64_t)n, vk, K, (int8_t*)v.out.p);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipEventRecord(v.ev1, v.stream));
    v.timed = true;
    ZK_HIP(hipMemcpyAsync(verdicts, v.out.p, n, hipMemcpyDeviceToHost, v.stream));
    ZK_HIP(hipStreamSynchronize(v.stream));
    return ZKMI_OK;
}

template <class C> int pairing_batch(const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t* out) {
    VerifyCtx& v = vctx();
    constexpr int N = C::N;
    const PairingConsts<C>* K;
    ZK_TRY(consts_dev<C>(&K));
    const size_t b1 = 3 * 4 * N, b2 = 6 * 4 * N, bo = 12 * 4 * N;
    ZK_TRY(grow(v.in_a, n * b1));
    ZK_TRY(grow(v.in_b, n * b2));
    ZK_TRY(grow(v.out, n * bo));
    ZK_HIP(hipMemcpyAsync(v.in_a.p, g1, n * b1, hipMemcpyHostToDevice, v.stream));
    ZK_HIP(hipMemcpyAsync(v.in_b.p, g2, n * b2, hipMemcpyHostToDevice, v.stream));
    hipLaunchKernelGGL(k_pairing<C>, dim3((unsigned)((n + VERIFY_BLOCK - 1) / VERIFY_BLOCK)), dim3(VERIFY_BLOCK), 0, v.stream, (const uint32_t*)v.in_a.p,
                       (const uint32_t*)v.in_b.p, (uint64_t)n, K, (Fp<C>*)v.out.p);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(out, v.out.p, n * bo, hipMemcpyDeviceToHost, v.stream));
    ZK_HIP(hipStreamSynchronize(v.stream));
    return ZKMI_OK;
}

}  // namespace
}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zkmi_groth16_vk_load(int curve, const uint8_t* alpha1_xyz, const uint8_t* beta2_xyz, const uint8_t* gamma2_xyz, const uint8_t* delta2_xyz,
                         const uint8_t* ic_xyz, uint32_t n_public, uint64_t* vk_handle) {
    std::lock_guard<std::mutex> g(vctx().mu);
    ZK_TRY(begin());
    if (!alpha1_xyz || !beta2_xyz || !gamma2_xyz || !delta2_xyz || !ic_xyz || !vk_handle) return fail(ZKMI_ERR_INVALID, "groth16_vk_load: null argument");
    if (curve == ZKMI_CURVE_BN128) return vk_load<Bn254Fq>(alpha1_xyz, beta2_xyz, gamma2_xyz, delta2_xyz, ic_xyz, n_public, vk_handle);
    if (curve == ZKMI_CURVE_BLS12381) return vk_load<Bls12381Fq>(alpha1_xyz, beta2_xyz, gamma2_xyz, delta2_xyz, ic_xyz, n_public, vk_handle);
    return fail(ZKMI_ERR_INVALID, "groth16_vk_load: unknown curve");
}

int zkmi_groth16_verify_batch(uint64_t vk_handle, const uint8_t* proofs_xyz, const uint8_t* publics, uint32_t n_signals, size_t n, int8_t* verdicts) {
    std::lock_guard<std::mutex> g(vctx().mu);
    ZK_TRY(begin());
    auto it = vctx().keys.find(vk_handle);
    if (it == vctx().keys.end()) return fail(ZKMI_ERR_INVALID, "groth16_verify_batch: unknown verifying key");
    const VkEntry& e = it->second;
    if (n_signals > e.n_public) return fail(ZKMI_ERR_INVALID, "groth16_verify_batch: more public signals than the key's nPublic");
    if (n == 0) return ZKMI_OK;
    if (!proofs_xyz || !verdicts || (n_signals && !publics)) return fail(ZKMI_ERR_INVALID, "groth16_verify_batch: null argument");
    if (e.curve == ZKMI_CURVE_BN128) return verify_batch<Bn254Fq>(e, proofs_xyz, publics, n_signals, n, verdicts);
    return verify_batch<Bls12381Fq>(e, proofs_xyz, publics, n_signals, n, verdicts);
}

double zkmi_groth16_verify_last_ms(void) {
    std::lock_guard<std::mutex> g(vctx().mu);
    VerifyCtx& v = vctx();
    float ms = 0;
    if (!v.timed || hipEventElapsedTime(&ms, v.ev0, v.ev1) != hipSuccess) return -1.0;
    return ms;
}

int zkmi_groth16_vk_release(uint64_t vk_handle) {
    std::lock_guard<std::mutex> g(vctx().mu);
    auto it = vctx().keys.find(vk_handle);
    if (it == vctx().keys.end()) return fail(ZKMI_ERR_INVALID, "groth16_vk_release: unknown verifying key");
    ZK_HIP(hipFree(it->second.d_ic));
    ZK_HIP(hipFree(it->second.d_tabs));
    ZK_HIP(hipFree(it->second.d_mab));
    vctx().keys.erase(it);
    return ZKMI_OK;
}

int zkmi_pairing_dev(int curve, const uint8_t* g1_xyz, const uint8_t* g2_xyz, size_t n, uint8_t* out_f12) {
    std::lock_guard<std::mutex> g(vctx().mu);
    ZK_TRY(begin());
    if (n == 0) return ZKMI_OK;
    if (!g1_xyz || !g2_xyz || !out_f12) return fail(ZKMI_ERR_INVALID, "pairing_dev: null argument");
    if (curve == ZKMI_CURVE_BN128) return pairing_batch<Bn254Fq>(g1_xyz, g2_xyz, n, out_f12);
    if (curve == ZKMI_CURVE_BLS12381) return pairing_batch<Bls12381Fq>(g1_xyz, g2_xyz, n, out_f12);
    return fail(ZKMI_ERR_INVALID, "pairing_dev: unknown curve");
}

}  // extern "C"
