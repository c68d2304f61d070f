// snarkjs_amd/csrc/groth16_verify.hip — batch Groth16 verification (src/groth16_verify.js:26-87) and the diagnostic pairing, gfx950.
//
// Per verifying key (zkmi_groth16_vk_load): the key's points go to Montgomery form and the line tables of beta, gamma, delta and the Miller
// value M(alpha, beta) are built once by one lane (pairing.cuh vk_prepare); every proof lane reads them. Per proof (one lane each):
// publics < r, pi_a / pi_b / pi_c on the curve (no subgroup check, as the reference), vk_x by interleaved double-and-add over the publics,
// the multi-Miller loop (pi_b walked, gamma and delta from their tables), times M(alpha, beta), the final exponentiation, == 1.
//
// The aggregated check of a whole batch (k_g16_agg_lane, k_g16_agg_reduce, k_g16_agg_tail here): groth16_aggregate.cuh.
//
// Isolation from the provers, and the one coupling through hipFree that remains: verify_host.hpp. This verifier's context is vctx().
#include <string.h>
#include "aggregate_host.hpp"
#include "groth16_aggregate.cuh"

namespace zkmi {
namespace {

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

// The 64 records of a block -> one, in LDS: the Fq12 values by a tree of f12_mul, then the pairs of sums by agg_block_sum in the SAME region
// (24 / 36 KB), then the sums of the challenges (1.5 KB). Every thread of the block must call it; thread 0 writes *out.
template <class C> constexpr size_t g16_lds_bytes() {
    return VERIFY_BLOCK * (sizeof(Fp12<C>) > sizeof(AggPair<C>) ? sizeof(Fp12<C>) : sizeof(AggPair<C>));
}
template <class C> __device__ __forceinline__ void g16_block_reduce(unsigned char* region, uint64_t* sh_r, const G16Part<C>& mine, G16Part<C>* out) {
    const unsigned t = threadIdx.x;
    Fp12<C>* sh_f = (Fp12<C>*)region;
    g16_block_prod<C, VERIFY_BLOCK>(sh_f, t, mine.f);
    if (t == 0) out->f = sh_f[0];
    __syncthreads();
    AggPair<C>* sh_s = (AggPair<C>*)region;
    agg_block_sum<C, VERIFY_BLOCK>(sh_s, t, mine.s);
    if (t == 0) out->s = sh_s[0];
    g16_block_add3<VERIFY_BLOCK>(sh_r, t, mine.r);
    if (t == 0)
        for (int k = 0; k < 3; k++) out->r[k] = sh_r[k];
}

// The lane phase of the aggregated check: one proof per lane (g16_agg_lane_one), one record per block.
template <class C> __global__ void __launch_bounds__(VERIFY_BLOCK) k_g16_agg_lane(const uint32_t* recs, const uint32_t* pubs, uint32_t n_sig, uint64_t n, VkView<C> vk,
                                                                                   const PairingConsts<C>* K, AggSeed seed, int8_t* out, G16Part<C>* parts) {
    __shared__ __attribute__((aligned(16))) unsigned char region[g16_lds_bytes<C>()];
    __shared__ uint64_t sh_r[3 * VERIFY_BLOCK];
    const uint64_t i = (uint64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    G16Part<C> mine;
    if (i < n) out[i] = (int8_t)g16_agg_lane_one(recs + i * 12 * C::N, pubs + i * 8 * n_sig, n_sig, vk, K, seed.w, i, mine);
    else g16_part_identity(mine);
    g16_block_reduce<C>(region, sh_r, mine, parts + blockIdx.x);
}

template <class C> __global__ void __launch_bounds__(VERIFY_BLOCK) k_g16_agg_reduce(const G16Part<C>* in, uint64_t m, G16Part<C>* out) {
    __shared__ __attribute__((aligned(16))) unsigned char region[g16_lds_bytes<C>()];
    __shared__ uint64_t sh_r[3 * VERIFY_BLOCK];
    const uint64_t i = (uint64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    G16Part<C> mine;
    if (i < m) mine = in[i];
    else g16_part_identity(mine);
    g16_block_reduce<C>(region, sh_r, mine, out + blockIdx.x);
}

template <class C> __global__ void __launch_bounds__(64) k_g16_agg_tail(const G16Part<C>* S, VkView<C> vk, const PairingConsts<C>* K, int trace, G16AggResult<C>* out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    g16_agg_tail(*S, vk, K, trace != 0, out);
}

struct VkEntry {
    int curve = 0;
    uint32_t n_public = 0, flags = 0;
    void* blocks[3] = {nullptr, nullptr, nullptr};         // IC (affine, Montgomery) | the line tables of beta, gamma, delta | M(alpha, beta)
};
KzgVerifyCtx<VkEntry>& vctx() {
    static KzgVerifyCtx<VkEntry> v;
    return v;
}

template <class C> int vk_build(VkEntry& e, const std::vector<uint8_t>& pts, size_t n_ic, const PairingConsts<C>* K) {
    auto& v = vctx();
    constexpr int NL = miller_lines<C>();
    ZK_HIP(hipMalloc(&e.blocks[0], n_ic * 2 * sizeof(Fp<C>)));
    ZK_HIP(hipMalloc(&e.blocks[1], 3 * NL * sizeof(Line<C>)));
    ZK_HIP(hipMalloc(&e.blocks[2], sizeof(Fp12<C>)));
    ZK_TRY(grow(v.in_a, pts.size()));
    ZK_TRY(grow(v.out, 16));
    ZK_HIP(hipMemcpyAsync(v.in_a.p, pts.data(), pts.size(), hipMemcpyHostToDevice, v.stream));
    hipLaunchKernelGGL(k_vk_prepare<C>, dim3(1), dim3(64), 0, v.stream, (const uint32_t*)v.in_a.p, (uint32_t)n_ic, K, (Fp<C>*)e.blocks[0], (Line<C>*)e.blocks[1],
                       (Fp12<C>*)e.blocks[2], (uint32_t*)v.out.p);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(&e.flags, v.out.p, 4, hipMemcpyDeviceToHost, v.stream));
    ZK_HIP(hipStreamSynchronize(v.stream));
    return ZKMI_OK;
}

template <class C> int vk_load(const uint8_t* alpha, const uint8_t* beta, const uint8_t* gamma, const uint8_t* delta, const uint8_t* ic, uint32_t n_public,
                               uint64_t* handle) {
    auto& v = vctx();
    constexpr int N = C::N;
    const PairingConsts<C>* K;
    ZK_TRY(v.consts<C>(&K));
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
    if (rc) return v.drop(e, rc);
    *handle = v.add(e);
    return ZKMI_OK;
}

template <class C> VkView<C> vk_view(const VkEntry& e) {
    constexpr int NL = miller_lines<C>();
    const Line<C>* tabs = (const Line<C>*)e.blocks[1];
    return VkView<C>{(const Fp<C>*)e.blocks[0], e.n_public + 1, tabs + NL, tabs + 2 * NL, e.flags & 1u, (e.flags >> 1) & 1u, (const Fp12<C>*)e.blocks[2]};
}

template <class C> int verify_batch(const VkEntry& e, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, int8_t* verdicts) {
    auto& v = vctx();
    constexpr int N = C::N;
    const PairingConsts<C>* K;
    ZK_TRY(v.consts<C>(&K));
    const VkView<C> vk = vk_view<C>(e);
    return v.run_batch(proofs, n * 12 * 4 * N, publics, n * n_signals * 32, verdicts, n, nullptr, 0, true, [&] {
        hipLaunchKernelGGL(k_g16_verify<C>, dim3(verify_grid(n)), dim3(VERIFY_BLOCK), 0, v.stream, (const uint32_t*)v.in_a.p, (const uint32_t*)v.in_b.p, n_signals,
                           (uint64_t)n, vk, K, (int8_t*)v.out.p);
    });
}

// One aggregated batch of n > 0 proofs, on the pattern of run_aggregate (aggregate_host.hpp): the lane kernel between ev0 and ev1, the reduction
// up to ev2, the tail up to ev3. codes (n) and *ok are filled; trace (may be null) receives S_X | S_C (4 n8q bytes) | s (24) | final_exp(F) (12 n8q).
template <class C> int aggregate_batch(const VkEntry& e, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, const uint8_t* seed, int8_t* codes,
                                       int* ok, uint8_t* trace) {
    auto& v = vctx();
    constexpr int N = C::N;
    const PairingConsts<C>* K;
    ZK_TRY(v.consts<C>(&K));
    const VkView<C> vk = vk_view<C>(e);
    AggSeed sd;
    memcpy(sd.w, seed, 32);
    const unsigned blocks = verify_grid(n);
    const size_t a_bytes = n * 12 * 4 * N, b_bytes = n * n_signals * 32;
    ZK_TRY(grow(v.in_a, a_bytes));
    ZK_TRY(grow(v.in_b, b_bytes + 32));
    ZK_TRY(grow(v.out, n));
    ZK_TRY(grow(v.agg_a, (size_t)blocks * sizeof(G16Part<C>)));
    ZK_TRY(grow(v.agg_b, (size_t)verify_grid(blocks) * sizeof(G16Part<C>)));
    ZK_TRY(grow(v.agg_res, sizeof(G16AggResult<C>)));
    ZK_HIP(hipMemcpyAsync(v.in_a.p, proofs, a_bytes, hipMemcpyHostToDevice, v.stream));
    if (b_bytes) ZK_HIP(hipMemcpyAsync(v.in_b.p, publics, b_bytes, hipMemcpyHostToDevice, v.stream));
    ZK_HIP(hipEventRecord(v.ev0, v.stream));
    G16Part<C>* src = (G16Part<C>*)v.agg_a.p;
    G16Part<C>* dst = (G16Part<C>*)v.agg_b.p;
    hipLaunchKernelGGL(k_g16_agg_lane<C>, dim3(blocks), dim3(VERIFY_BLOCK), 0, v.stream, (const uint32_t*)v.in_a.p, (const uint32_t*)v.in_b.p, n_signals, (uint64_t)n, vk, K,
                       sd, (int8_t*)v.out.p, src);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipEventRecord(v.ev1, v.stream));
    for (unsigned m = blocks; m > 1;) {
        const unsigned g = verify_grid(m);
        hipLaunchKernelGGL(k_g16_agg_reduce<C>, dim3(g), dim3(VERIFY_BLOCK), 0, v.stream, (const G16Part<C>*)src, (uint64_t)m, dst);
        ZK_HIP(hipGetLastError());
        G16Part<C>* t = src; src = dst; dst = t;
        m = g;
    }
    ZK_HIP(hipEventRecord(v.ev2, v.stream));
    hipLaunchKernelGGL(k_g16_agg_tail<C>, dim3(1), dim3(64), 0, v.stream, (const G16Part<C>*)src, vk, K, trace ? 1 : 0, (G16AggResult<C>*)v.agg_res.p);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipEventRecord(v.ev3, v.stream));
    v.timed = true;
    v.agg_last = true;
    // res is on this frame: whatever the copies return, the stream is idle before the function is left
    G16AggResult<C> res;
    hipError_t copied = hipMemcpyAsync(codes, v.out.p, n, hipMemcpyDeviceToHost, v.stream);
    if (copied == hipSuccess) copied = hipMemcpyAsync(&res, v.agg_res.p, sizeof res, hipMemcpyDeviceToHost, v.stream);
    const hipError_t idle = hipStreamSynchronize(v.stream);
    ZK_HIP(copied);
    ZK_HIP(idle);
    bool all = res.pair_ok != 0;
    for (size_t i = 0; i < n; i++) all = all && codes[i] == AGG_ENTERED;
    *ok = all ? 1 : 0;
    if (trace) {
        memcpy(trace, res.sx, 8 * N);
        memcpy(trace + 8 * N, res.sc, 8 * N);
        memcpy(trace + 16 * N, res.s, 24);
        memcpy(trace + 16 * N + 24, res.gt, 48 * N);
    }
    return ZKMI_OK;
}

// the aggregated entry: the same refusals as zkmi_groth16_verify_batch; an empty batch is ok; trace (may be null) is zeroed first, and final_exp of
// the empty product is one
int aggregate_entry(const char* who, uint64_t vk_handle, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, const uint8_t* seed, int8_t* codes, int* ok,
                    uint8_t* trace) {
    ZK_TRY(vctx().begin());
    const VkEntry* e = vctx().find(vk_handle, who);
    if (!e) return ZKMI_ERR_INVALID;
    if (n_signals > e->n_public) return fail(ZKMI_ERR_INVALID, std::string(who) + ": more public signals than the key's nPublic");
    if (!seed || !ok) return fail(ZKMI_ERR_INVALID, std::string(who) + ": null argument");
    const size_t n8 = e->curve == ZKMI_CURVE_BN128 ? 32 : 48;
    if (trace) {
        memset(trace, 0, 16 * n8 + 24);
        trace[4 * n8 + 24] = 1;
    }
    *ok = 1;
    if (n == 0) return ZKMI_OK;
    *ok = 0;
    if (!proofs || !codes || (n_signals && !publics)) return fail(ZKMI_ERR_INVALID, std::string(who) + ": null argument");
    if (e->curve == ZKMI_CURVE_BN128) return aggregate_batch<Bn254Fq>(*e, proofs, publics, n_signals, n, seed, codes, ok, trace);
    return aggregate_batch<Bls12381Fq>(*e, proofs, publics, n_signals, n, seed, codes, ok, trace);
}

// untimed: zkmi_groth16_verify_last_ms keeps reporting the last verify kernel
template <class C> int pairing_batch(const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t* out) {
    auto& v = vctx();
    constexpr int N = C::N;
    const PairingConsts<C>* K;
    ZK_TRY(v.consts<C>(&K));
    return v.run_batch(g1, n * 3 * 4 * N, g2, n * 6 * 4 * N, out, n * 12 * 4 * N, nullptr, 0, false, [&] {
        hipLaunchKernelGGL(k_pairing<C>, dim3(verify_grid(n)), dim3(VERIFY_BLOCK), 0, v.stream, (const uint32_t*)v.in_a.p, (const uint32_t*)v.in_b.p, (uint64_t)n, K,
                           (Fp<C>*)v.out.p);
    });
}

}  // namespace
}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zkmi_groth16_vk_load(int curve, const uint8_t* alpha1_xyz, const uint8_t* beta2_xyz, const uint8_t* gamma2_xyz, const uint8_t* delta2_xyz,
                         const uint8_t* ic_xyz, uint32_t n_public, uint64_t* vk_handle) {
    std::lock_guard<std::mutex> g(vctx().mu);
    ZK_TRY(vctx().begin());
    if (!alpha1_xyz || !beta2_xyz || !gamma2_xyz || !delta2_xyz || !ic_xyz || !vk_handle) return fail(ZKMI_ERR_INVALID, "groth16_vk_load: null argument");
    if (curve == ZKMI_CURVE_BN128) return vk_load<Bn254Fq>(alpha1_xyz, beta2_xyz, gamma2_xyz, delta2_xyz, ic_xyz, n_public, vk_handle);
    if (curve == ZKMI_CURVE_BLS12381) return vk_load<Bls12381Fq>(alpha1_xyz, beta2_xyz, gamma2_xyz, delta2_xyz, ic_xyz, n_public, vk_handle);
    return fail(ZKMI_ERR_INVALID, "groth16_vk_load: unknown curve");
}

int zkmi_groth16_verify_batch(uint64_t vk_handle, const uint8_t* proofs_xyz, const uint8_t* publics, uint32_t n_signals, size_t n, int8_t* verdicts) {
    std::lock_guard<std::mutex> g(vctx().mu);
    ZK_TRY(vctx().begin());
    const VkEntry* e = vctx().find(vk_handle, "groth16_verify_batch");
    if (!e) return ZKMI_ERR_INVALID;
    if (n_signals > e->n_public) return fail(ZKMI_ERR_INVALID, "groth16_verify_batch: more public signals than the key's nPublic");
    if (n == 0) return ZKMI_OK;
    if (!proofs_xyz || !verdicts || (n_signals && !publics)) return fail(ZKMI_ERR_INVALID, "groth16_verify_batch: null argument");
    if (e->curve == ZKMI_CURVE_BN128) return verify_batch<Bn254Fq>(*e, proofs_xyz, publics, n_signals, n, verdicts);
    return verify_batch<Bls12381Fq>(*e, proofs_xyz, publics, n_signals, n, verdicts);
}

int zkmi_groth16_verify_aggregate(uint64_t vk_handle, const uint8_t* proofs_xyz, const uint8_t* publics, uint32_t n_signals, size_t n, const uint8_t seed[32], int8_t* codes,
                                  int* ok) {
    std::lock_guard<std::mutex> g(vctx().mu);
    return aggregate_entry("groth16_verify_aggregate", vk_handle, proofs_xyz, publics, n_signals, n, seed, codes, ok, nullptr);
}

int zkmi_groth16_aggregate_trace_dev(uint64_t vk_handle, const uint8_t* proofs_xyz, const uint8_t* publics, uint32_t n_signals, size_t n, const uint8_t seed[32], int8_t* codes,
                                     int* ok, uint8_t* trace) {
    std::lock_guard<std::mutex> g(vctx().mu);
    if (!trace) return fail(ZKMI_ERR_INVALID, "groth16_aggregate_trace_dev: null argument");
    return aggregate_entry("groth16_aggregate_trace_dev", vk_handle, proofs_xyz, publics, n_signals, n, seed, codes, ok, trace);
}

int zkmi_groth16_aggregate_phase_ms(double* lane_reduce_tail) {
    std::lock_guard<std::mutex> g(vctx().mu);
    return vctx().phase_ms("groth16_aggregate_phase_ms", lane_reduce_tail);
}

double zkmi_groth16_verify_last_ms(void) {
    std::lock_guard<std::mutex> g(vctx().mu);
    return vctx().last_ms();
}

int zkmi_groth16_vk_release(uint64_t vk_handle) {
    std::lock_guard<std::mutex> g(vctx().mu);
    return vctx().release(vk_handle, "groth16_vk_release");
}

int zkmi_pairing_dev(int curve, const uint8_t* g1_xyz, const uint8_t* g2_xyz, size_t n, uint8_t* out_f12) {
    std::lock_guard<std::mutex> g(vctx().mu);
    ZK_TRY(vctx().begin());
    if (n == 0) return ZKMI_OK;
    if (!g1_xyz || !g2_xyz || !out_f12) return fail(ZKMI_ERR_INVALID, "pairing_dev: null argument");
    if (curve == ZKMI_CURVE_BN128) return pairing_batch<Bn254Fq>(g1_xyz, g2_xyz, n, out_f12);
    if (curve == ZKMI_CURVE_BLS12381) return pairing_batch<Bls12381Fq>(g1_xyz, g2_xyz, n, out_f12);
    return fail(ZKMI_ERR_INVALID, "pairing_dev: unknown curve");
}

}  // extern "C"
