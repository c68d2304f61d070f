// snarkjs_amd/csrc/fflonk_verify.hip — batch FFLONK verification (src/fflonk_verify.js:28-137) on the device, gfx950, BN254.
//
// Per verifying key (zkmi_fflonk_vk_load): one lane brings C0 to Montgomery form with its on-curve flag and its transcript bytes, checks X_2 on
// its curve, builds the line tables of X_2 and of the G2 generator and the Fr constants (k1 k2 wr, w = Fr.w[power], 1/n, the powers of w8 w4 w3)
// — fflonk_verify.cuh fflonk_vk_prepare. Per proof (one lane each): fflonk_verify_one — input checks, the Keccak-256 transcript, the Fr part
// with one batched inversion, A1 by one five-base Straus sum, the two-table Miller loop, the final exponentiation.
//
// BLS12-381 is refused: the reference's fflonk.setup / fflonk.prove do not work on it, so there is no verdict to hold one to.
//
// The aggregated check of a whole batch (k_fflonk_agg_lane here, then the reduction and the tail of aggregate_host.hpp): kzg_aggregate.cuh.
//
// Isolation from the provers and the other verifiers, and the one coupling through hipFree that remains: verify_host.hpp. This verifier's
// context is fctx().
#include <stddef.h>
#include <string.h>
#include "aggregate_host.hpp"
#include "fflonk_verify.cuh"

namespace zkmi {
namespace {

template <class C> __global__ void __launch_bounds__(64) k_fflonk_vk_prepare(const uint32_t* in, uint32_t power, uint32_t n_public, const PairingConsts<C>* K, FflonkVk<C>* vk,
                                                                             Line<C>* tabs) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    constexpr int N = C::N;
    // in: C0 (3 Fq), X_2 (3 Fq2), k1 k2 w3 w4 w8 wr, omega (8 words each)
    fflonk_vk_prepare(in, in + 3 * N, in + 9 * N, in + 9 * N + 48, power, n_public, K, vk, tabs, tabs + miller_lines<C>());
}

template <class C> __global__ void __launch_bounds__(VERIFY_BLOCK) k_fflonk_verify(const uint32_t* recs, const uint32_t* pubs, uint64_t n, FflonkVkView<C> V,
                                                                                         const PairingConsts<C>* K, int8_t* out, FflonkTrace<C>* tr) {
    const uint64_t i = (uint64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = (int8_t)fflonk_verify_one(recs + i * fflonk_record_words<C>(), pubs + i * 8 * V.vk->n_public, V, K, tr);
}

// The lane phase of the aggregated check (kzg_aggregate.cuh): fflonk_verify_one up to its two points, then r_i times the lane's pair; the block's 64 pairs are added
// in LDS and leave as one (aggregate_host.hpp agg_lane).
template <class C> __global__ void __launch_bounds__(VERIFY_BLOCK) k_fflonk_agg_lane(const uint32_t* recs, const uint32_t* pubs, uint64_t n, FflonkVkView<C> V,
                                                                                           const PairingConsts<C>* K, AggSeed seed, int8_t* out, AggPair<C>* parts) {
    __shared__ AggPair<C> sh[VERIFY_BLOCK];
    agg_lane<C>(sh, n, seed, out, parts, [&](uint64_t i, KzgPair<C>* pr) {
        return fflonk_verify_one<C, true>(recs + i * fflonk_record_words<C>(), pubs + i * 8 * V.vk->n_public, V, K, (FflonkTrace<C>*)nullptr, pr);
    });
}

struct FflonkVkEntry {
    int curve = 0;
    uint32_t n_public = 0;
    void* blocks[2] = {nullptr, nullptr};                  // FflonkVk | the line tables of X_2 and of the G2 generator
};
KzgVerifyCtx<FflonkVkEntry>& fctx() {
    static KzgVerifyCtx<FflonkVkEntry> v;
    return v;
}

template <class C> int vk_build(FflonkVkEntry& e, const std::vector<uint8_t>& in, uint32_t power, uint32_t n_public, uint32_t* bad) {
    auto& v = fctx();
    const PairingConsts<C>* K;
    ZK_TRY(v.consts<C>(&K));
    ZK_HIP(hipMalloc(&e.blocks[0], sizeof(FflonkVk<C>)));
    ZK_HIP(hipMalloc(&e.blocks[1], 2 * miller_lines<C>() * sizeof(Line<C>)));
    ZK_TRY(grow(v.in_a, in.size()));
    ZK_HIP(hipMemcpyAsync(v.in_a.p, in.data(), in.size(), hipMemcpyHostToDevice, v.stream));
    hipLaunchKernelGGL(k_fflonk_vk_prepare<C>, dim3(1), dim3(64), 0, v.stream, (const uint32_t*)v.in_a.p, power, n_public, K, (FflonkVk<C>*)e.blocks[0], (Line<C>*)e.blocks[1]);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(bad, (const uint8_t*)e.blocks[0] + offsetof(FflonkVk<C>, bad), 4, hipMemcpyDeviceToHost, v.stream));
    ZK_HIP(hipStreamSynchronize(v.stream));
    return ZKMI_OK;
}

template <class C> int vk_load(const uint8_t* c0, const uint8_t* x2, const uint8_t* consts, uint32_t power, uint32_t n_public, uint64_t* handle) {
    auto& v = fctx();
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
    if (rc) return v.drop(e, rc);
    *handle = v.add(e);
    return ZKMI_OK;
}

template <class C> int verify_batch(const FflonkVkEntry& e, const uint8_t* proofs, const uint8_t* publics, size_t n, int8_t* verdicts, uint8_t* trace_out) {
    auto& v = fctx();
    const PairingConsts<C>* K;
    ZK_TRY(v.consts<C>(&K));
    const Line<C>* tabs = (const Line<C>*)e.blocks[1];
    const FflonkVkView<C> V{(const FflonkVk<C>*)e.blocks[0], tabs, tabs + miller_lines<C>()};
    return v.run_batch(proofs, n * 4 * fflonk_record_words<C>(), publics, n * e.n_public * 32, verdicts, n, trace_out, sizeof(FflonkTrace<C>), true, [&] {
        hipLaunchKernelGGL(k_fflonk_verify<C>, dim3(verify_grid(n)), dim3(VERIFY_BLOCK), 0, v.stream, (const uint32_t*)v.in_a.p, (const uint32_t*)v.in_b.p, (uint64_t)n, V, K,
                           (int8_t*)v.out.p, trace_out ? (FflonkTrace<C>*)v.trace.p : nullptr);
    });
}

int verify_entry(const char* who, uint64_t vk_handle, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, int8_t* verdicts, uint8_t* trace_out) {
    ZK_TRY(fctx().begin());
    const FflonkVkEntry* found = fctx().find(vk_handle, who);
    if (!found) return ZKMI_ERR_INVALID;
    const FflonkVkEntry& e = *found;
    if (n_signals != e.n_public) return fail(ZKMI_ERR_INVALID, "Number of public signals does not match with vk");
    if (n == 0) return ZKMI_OK;
    if (!proofs || !verdicts || (n_signals && !publics)) return fail(ZKMI_ERR_INVALID, std::string(who) + ": null argument");
    return verify_batch<Bn254Fq>(e, proofs, publics, n, verdicts, trace_out);
}

template <class C> int aggregate_batch(const FflonkVkEntry& e, const uint8_t* proofs, const uint8_t* publics, size_t n, const uint8_t* seed, int8_t* codes, int* ok, uint8_t* sums) {
    auto& v = fctx();
    const PairingConsts<C>* K;
    ZK_TRY(v.consts<C>(&K));
    const Line<C>* tabs = (const Line<C>*)e.blocks[1];
    const FflonkVkView<C> V{(const FflonkVk<C>*)e.blocks[0], tabs, tabs + miller_lines<C>()};
    AggSeed sd;
    memcpy(sd.w, seed, 32);
    const uint32_t* x2_inf = (const uint32_t*)((const uint8_t*)e.blocks[0] + offsetof(FflonkVk<C>, x2_inf));
    return run_aggregate<C>(v, proofs, n * 4 * fflonk_record_words<C>(), publics, n * e.n_public * 32, n, codes, ok, sums, tabs + miller_lines<C>(), tabs, x2_inf, 0, K,
                                   [&](unsigned blocks, AggPair<C>* parts) {
        hipLaunchKernelGGL(k_fflonk_agg_lane<C>, dim3(blocks), dim3(VERIFY_BLOCK), 0, v.stream, (const uint32_t*)v.in_a.p, (const uint32_t*)v.in_b.p, (uint64_t)n, V, K, sd,
                           (int8_t*)v.out.p, parts);
    });
}

// the aggregated entry: the same refusals as verify_entry; an empty batch is ok; sums (may be null) is zeroed first
int aggregate_entry(const char* who, uint64_t vk_handle, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, const uint8_t* seed, int8_t* codes, int* ok,
                    uint8_t* sums) {
    ZK_TRY(fctx().begin());
    const FflonkVkEntry* found = fctx().find(vk_handle, who);
    if (!found) return ZKMI_ERR_INVALID;
    const FflonkVkEntry& e = *found;
    if (n_signals != e.n_public) return fail(ZKMI_ERR_INVALID, "Number of public signals does not match with vk");
    if (!seed || !ok) return fail(ZKMI_ERR_INVALID, std::string(who) + ": null argument");
    if (sums) memset(sums, 0, e.curve == ZKMI_CURVE_BN128 ? 128 : 192);
    *ok = 1;
    if (n == 0) return ZKMI_OK;
    *ok = 0;
    if (!proofs || !codes || (n_signals && !publics)) return fail(ZKMI_ERR_INVALID, std::string(who) + ": null argument");
    return aggregate_batch<Bn254Fq>(e, proofs, publics, n, seed, codes, ok, sums);
}

}  // namespace
}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zkmi_fflonk_vk_load(int curve, const uint8_t* c0_xyz, const uint8_t* x2_xyz, const uint8_t* consts, uint32_t power, uint32_t n_public, uint64_t* vk_handle) {
    std::lock_guard<std::mutex> g(fctx().mu);
    ZK_TRY(fctx().begin());
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

int zkmi_fflonk_verify_aggregate(uint64_t vk_handle, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, const uint8_t seed[32], int8_t* codes, int* ok) {
    std::lock_guard<std::mutex> g(fctx().mu);
    return aggregate_entry("fflonk_verify_aggregate", vk_handle, proofs, publics, n_signals, n, seed, codes, ok, nullptr);
}

int zkmi_fflonk_aggregate_trace_dev(uint64_t vk_handle, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, const uint8_t seed[32], int8_t* codes, int* ok,
                                   uint8_t* sums) {
    std::lock_guard<std::mutex> g(fctx().mu);
    if (!sums) return fail(ZKMI_ERR_INVALID, "fflonk_aggregate_trace_dev: null argument");
    return aggregate_entry("fflonk_aggregate_trace_dev", vk_handle, proofs, publics, n_signals, n, seed, codes, ok, sums);
}

int zkmi_fflonk_aggregate_phase_ms(double* lane_reduce_tail) {
    std::lock_guard<std::mutex> g(fctx().mu);
    return fctx().phase_ms("fflonk_aggregate_phase_ms", lane_reduce_tail);
}

int zkmi_fflonk_vk_info(uint64_t vk_handle, int* curve, uint32_t* n_public) {
    std::lock_guard<std::mutex> g(fctx().mu);
    return fctx().info(vk_handle, "fflonk_vk_info", curve, n_public);
}

double zkmi_fflonk_verify_last_ms(void) {
    std::lock_guard<std::mutex> g(fctx().mu);
    return fctx().last_ms();
}

int zkmi_fflonk_vk_release(uint64_t vk_handle) {
    std::lock_guard<std::mutex> g(fctx().mu);
    return fctx().release(vk_handle, "fflonk_vk_release");
}

}  // extern "C"
