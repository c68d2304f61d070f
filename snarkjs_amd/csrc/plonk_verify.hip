// snarkjs_amd/csrc/plonk_verify.hip — batch PLONK verification (src/plonk_verify.js:29-123) on the device, gfx950.
//
// Per verifying key (zkmi_plonk_vk_load): one lane brings the eight key points to Montgomery form, checks them and X_2 on their curves, builds
// the line tables of X_2 and of the G2 generator and the Fr constants (w = Fr.w[power], 1/n, k1, k2) — plonk_verify.cuh plonk_vk_prepare.
// Per proof (one lane each): plonk_verify_one — input checks, the Keccak-256 transcript, the Fr part, B1 by one 18-base Straus sum, A1, the
// two-table Miller loop, the final exponentiation.
//
// The aggregated check of a whole batch (k_plonk_agg_lane here, then the reduction and the tail of aggregate_host.hpp): kzg_aggregate.cuh.
//
// Isolation from the provers and the other verifiers, and the one coupling through hipFree that remains: verify_host.hpp. This verifier's
// context is pctx().
#include <stddef.h>
#include <string.h>
#include "aggregate_host.hpp"
#include "plonk_verify.cuh"

namespace zkmi {
namespace {

template <class C> __global__ void __launch_bounds__(64) k_plonk_vk_prepare(const uint32_t* in, uint32_t power, uint32_t n_public, const PairingConsts<C>* K, PlonkVk<C>* vk,
                                                                             Line<C>* tabs) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    constexpr int N = C::N;
    // in: eight G1 points (3 Fq each), X_2 (3 Fq2), k1, k2, omega (8 words each)
    plonk_vk_prepare(in, in + 24 * N, in + 30 * N, in + 30 * N + 8, in + 30 * N + 16, power, n_public, K, vk, tabs, tabs + miller_lines<C>());
}

template <class C> __global__ void __launch_bounds__(VERIFY_BLOCK) k_plonk_verify(const uint32_t* recs, const uint32_t* pubs, uint64_t n, PlonkVkView<C> V,
                                                                                         const PairingConsts<C>* K, int8_t* out, PlonkTrace<C>* tr) {
    const uint64_t i = (uint64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = (int8_t)plonk_verify_one(recs + i * plonk_record_words<C>(), pubs + i * 8 * V.vk->n_public, V, K, tr);
}

// The lane phase of the aggregated check (kzg_aggregate.cuh): plonk_verify_one up to its two points, then r_i times the lane's pair; the block's 64 pairs are added
// in LDS and leave as one (aggregate_host.hpp agg_lane).
template <class C> __global__ void __launch_bounds__(VERIFY_BLOCK) k_plonk_agg_lane(const uint32_t* recs, const uint32_t* pubs, uint64_t n, PlonkVkView<C> V,
                                                                                           const PairingConsts<C>* K, AggSeed seed, int8_t* out, AggPair<C>* parts) {
    __shared__ AggPair<C> sh[VERIFY_BLOCK];
    agg_lane<C>(sh, n, seed, out, parts, [&](uint64_t i, KzgPair<C>* pr) {
        return plonk_verify_one<C, true>(recs + i * plonk_record_words<C>(), pubs + i * 8 * V.vk->n_public, V, K, (PlonkTrace<C>*)nullptr, pr);
    });
}

struct PlonkVkEntry {
    int curve = 0;
    uint32_t n_public = 0;
    void* blocks[2] = {nullptr, nullptr};                  // PlonkVk | the line tables of X_2 and of the G2 generator
};
KzgVerifyCtx<PlonkVkEntry>& pctx() {
    static KzgVerifyCtx<PlonkVkEntry> v;
    return v;
}

template <class C> int vk_build(PlonkVkEntry& e, const std::vector<uint8_t>& in, uint32_t power, uint32_t n_public, uint32_t* bad) {
    auto& v = pctx();
    const PairingConsts<C>* K;
    ZK_TRY(v.consts<C>(&K));
    ZK_HIP(hipMalloc(&e.blocks[0], sizeof(PlonkVk<C>)));
    ZK_HIP(hipMalloc(&e.blocks[1], 2 * miller_lines<C>() * sizeof(Line<C>)));
    ZK_TRY(grow(v.in_a, in.size()));
    ZK_HIP(hipMemcpyAsync(v.in_a.p, in.data(), in.size(), hipMemcpyHostToDevice, v.stream));
    hipLaunchKernelGGL(k_plonk_vk_prepare<C>, dim3(1), dim3(64), 0, v.stream, (const uint32_t*)v.in_a.p, power, n_public, K, (PlonkVk<C>*)e.blocks[0], (Line<C>*)e.blocks[1]);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(bad, (const uint8_t*)e.blocks[0] + offsetof(PlonkVk<C>, bad), 4, hipMemcpyDeviceToHost, v.stream));
    ZK_HIP(hipStreamSynchronize(v.stream));
    return ZKMI_OK;
}

template <class C> int vk_load(const uint8_t* g1, const uint8_t* x2, const uint8_t* k1, const uint8_t* k2, uint32_t power, uint32_t n_public, uint64_t* handle) {
    auto& v = pctx();
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
    if (rc) return v.drop(e, rc);
    *handle = v.add(e);
    return ZKMI_OK;
}

template <class C> int verify_batch(const PlonkVkEntry& e, const uint8_t* proofs, const uint8_t* publics, size_t n, int8_t* verdicts, uint8_t* trace_out) {
    auto& v = pctx();
    const PairingConsts<C>* K;
    ZK_TRY(v.consts<C>(&K));
    const Line<C>* tabs = (const Line<C>*)e.blocks[1];
    const PlonkVkView<C> V{(const PlonkVk<C>*)e.blocks[0], tabs, tabs + miller_lines<C>()};
    return v.run_batch(proofs, n * 4 * plonk_record_words<C>(), publics, n * e.n_public * 32, verdicts, n, trace_out, sizeof(PlonkTrace<C>), true, [&] {
        hipLaunchKernelGGL(k_plonk_verify<C>, dim3(verify_grid(n)), dim3(VERIFY_BLOCK), 0, v.stream, (const uint32_t*)v.in_a.p, (const uint32_t*)v.in_b.p, (uint64_t)n, V, K,
                           (int8_t*)v.out.p, trace_out ? (PlonkTrace<C>*)v.trace.p : nullptr);
    });
}

int verify_entry(const char* who, uint64_t vk_handle, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, int8_t* verdicts, uint8_t* trace_out) {
    ZK_TRY(pctx().begin());
    const PlonkVkEntry* found = pctx().find(vk_handle, who);
    if (!found) return ZKMI_ERR_INVALID;
    const PlonkVkEntry& e = *found;
    if (n_signals != e.n_public) return fail(ZKMI_ERR_INVALID, "Invalid number of public inputs");
    if (n == 0) return ZKMI_OK;
    if (!proofs || !verdicts || (n_signals && !publics)) return fail(ZKMI_ERR_INVALID, std::string(who) + ": null argument");
    if (e.curve == ZKMI_CURVE_BN128) return verify_batch<Bn254Fq>(e, proofs, publics, n, verdicts, trace_out);
    return verify_batch<Bls12381Fq>(e, proofs, publics, n, verdicts, trace_out);
}

template <class C> int aggregate_batch(const PlonkVkEntry& e, const uint8_t* proofs, const uint8_t* publics, size_t n, const uint8_t* seed, int8_t* codes, int* ok, uint8_t* sums) {
    auto& v = pctx();
    const PairingConsts<C>* K;
    ZK_TRY(v.consts<C>(&K));
    const Line<C>* tabs = (const Line<C>*)e.blocks[1];
    const PlonkVkView<C> V{(const PlonkVk<C>*)e.blocks[0], tabs, tabs + miller_lines<C>()};
    AggSeed sd;
    memcpy(sd.w, seed, 32);
    const uint32_t* x2_inf = (const uint32_t*)((const uint8_t*)e.blocks[0] + offsetof(PlonkVk<C>, x2_inf));
    return run_aggregate<C>(v, proofs, n * 4 * plonk_record_words<C>(), publics, n * e.n_public * 32, n, codes, ok, sums, tabs, tabs + miller_lines<C>(), x2_inf, 1, K,
                                   [&](unsigned blocks, AggPair<C>* parts) {
        hipLaunchKernelGGL(k_plonk_agg_lane<C>, dim3(blocks), dim3(VERIFY_BLOCK), 0, v.stream, (const uint32_t*)v.in_a.p, (const uint32_t*)v.in_b.p, (uint64_t)n, V, K, sd,
                           (int8_t*)v.out.p, parts);
    });
}

// the aggregated entry: the same refusals as verify_entry; an empty batch is ok; sums (may be null) is zeroed first
int aggregate_entry(const char* who, uint64_t vk_handle, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, const uint8_t* seed, int8_t* codes, int* ok,
                    uint8_t* sums) {
    ZK_TRY(pctx().begin());
    const PlonkVkEntry* found = pctx().find(vk_handle, who);
    if (!found) return ZKMI_ERR_INVALID;
    const PlonkVkEntry& e = *found;
    if (n_signals != e.n_public) return fail(ZKMI_ERR_INVALID, "Invalid number of public inputs");
    if (!seed || !ok) return fail(ZKMI_ERR_INVALID, std::string(who) + ": null argument");
    if (sums) memset(sums, 0, e.curve == ZKMI_CURVE_BN128 ? 128 : 192);
    *ok = 1;
    if (n == 0) return ZKMI_OK;
    *ok = 0;
    if (!proofs || !codes || (n_signals && !publics)) return fail(ZKMI_ERR_INVALID, std::string(who) + ": null argument");
    if (e.curve == ZKMI_CURVE_BN128) return aggregate_batch<Bn254Fq>(e, proofs, publics, n, seed, codes, ok, sums);
    return aggregate_batch<Bls12381Fq>(e, proofs, publics, n, seed, codes, ok, sums);
}

}  // namespace
}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zkmi_plonk_vk_load(int curve, const uint8_t* g1_points_xyz, const uint8_t* x2_xyz, const uint8_t* k1, const uint8_t* k2, uint32_t power, uint32_t n_public,
                       uint64_t* vk_handle) {
    std::lock_guard<std::mutex> g(pctx().mu);
    ZK_TRY(pctx().begin());
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

int zkmi_plonk_verify_aggregate(uint64_t vk_handle, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, const uint8_t seed[32], int8_t* codes, int* ok) {
    std::lock_guard<std::mutex> g(pctx().mu);
    return aggregate_entry("plonk_verify_aggregate", vk_handle, proofs, publics, n_signals, n, seed, codes, ok, nullptr);
}

int zkmi_plonk_aggregate_trace_dev(uint64_t vk_handle, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, const uint8_t seed[32], int8_t* codes, int* ok,
                                   uint8_t* sums) {
    std::lock_guard<std::mutex> g(pctx().mu);
    if (!sums) return fail(ZKMI_ERR_INVALID, "plonk_aggregate_trace_dev: null argument");
    return aggregate_entry("plonk_aggregate_trace_dev", vk_handle, proofs, publics, n_signals, n, seed, codes, ok, sums);
}

int zkmi_plonk_aggregate_phase_ms(double* lane_reduce_tail) {
    std::lock_guard<std::mutex> g(pctx().mu);
    return pctx().phase_ms("plonk_aggregate_phase_ms", lane_reduce_tail);
}

int zkmi_plonk_vk_info(uint64_t vk_handle, int* curve, uint32_t* n_public) {
    std::lock_guard<std::mutex> g(pctx().mu);
    return pctx().info(vk_handle, "plonk_vk_info", curve, n_public);
}

double zkmi_plonk_verify_last_ms(void) {
    std::lock_guard<std::mutex> g(pctx().mu);
    return pctx().last_ms();
}

int zkmi_plonk_vk_release(uint64_t vk_handle) {
    std::lock_guard<std::mutex> g(pctx().mu);
    return pctx().release(vk_handle, "plonk_vk_release");
}

}  // extern "C"
