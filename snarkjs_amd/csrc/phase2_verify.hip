// snarkjs_amd/csrc/phase2_verify.hip — host driver + C-ABI of what zKey.verifyFromInit / verifyFromR1cs compute on curve points (src/zkey_verify_frominit.js;
// DESIGN.md 17): the reference's keystream and its Fr.fromRng on the device (chacha.cuh), misc.sameRatio for a batch of point quadruples in one launch
// (the Miller loop and the final exponentiation of pairing.cuh), and the two sums of the L and of the H check (the MSM of msm*.hip with the scalars made on
// the device, k_setup_hdiff / k_setup_affine for batchSubtract, the transform with its fused pre-scale for batchApplyKey + fft).
#include <string.h>
#include "chacha.cuh"
#include "groth16_setup.cuh"
#include "host_field.hpp"
#include "pairing.cuh"
#include "pairing_host.hpp"
#include "phase2_host.hpp"
#include "setup_common.hpp"
#include "zkmi_common.hpp"

namespace zkmi {
namespace {

constexpr int SR_BLOCK = 64;                       // lanes per block of the same-ratio kernel, as the per-proof kernels of the verifiers

// verdict[i] = e(g1s, g2sx) e(-g1sx, g2s) == 1; any of the four at infinity: 0, nothing paired (src/misc.js:129-137)
template <class C> __global__ void __launch_bounds__(SR_BLOCK) k_same_ratio(const uint32_t* __restrict__ g1s, const uint32_t* __restrict__ g1sx, const uint32_t* __restrict__ g2s,
                                                                            const uint32_t* __restrict__ g2sx, uint64_t n, const PairingConsts<C>* K, int8_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * SR_BLOCK + threadIdx.x;
    if (i >= n) return;
    Affine<Fp<C>> P, Px;
    Affine<Fp2<C>> Q, Qx;
    pt_load(P, g1s + i * 2 * C::N); pt_load(Px, g1sx + i * 2 * C::N);
    pt_load(Q, g2s + i * 4 * C::N); pt_load(Qx, g2sx + i * 4 * C::N);
    if (pt_is_inf(P) || pt_is_inf(Px) || pt_is_inf(Q) || pt_is_inf(Qx)) { out[i] = 0; return; }
    const FixedPair<C> none{nullptr, P.x, P.y, false};
    // a pair is handed over as (-x, y) of its G1 point: g1s = (x, y) -> (-x, y); -g1sx = (x, -y) -> (-x, -y)
    Fp12<C> f = miller_multi(Qx, fp_neg(P.x), P.y, true, none, none, K);
    f = f12_mul(f, miller_multi(Q, fp_neg(Px.x), fp_neg(Px.y), true, none, none, K));
    // final_exp_chain is final_exp to a fixed power coprime to r (pairing.cuh): "is one" is the same question, by three (BN254) or five (BLS12-381) powers of
    // x on cyclotomic squarings instead of ~760 / ~1270 full squarings. One lane's latency IS the time of the launch here, so the shorter chain is taken.
    out[i] = f12_is_one(final_exp_chain(f, K)) ? 1 : 0;
}

void* g_pairing_consts[2] = {nullptr, nullptr};
template <class C> int pairing_consts_dev(const PairingConsts<C>** out) {
    const int ci = C::N == 8 ? 0 : 1;
    if (!g_pairing_consts[ci]) {
        PairingConsts<C> K;
        pairing_consts_host(K);
        void* d = nullptr;
        ZK_HIP(hipMalloc(&d, sizeof K));
        hipError_t e = hipMemcpyAsync(d, &K, sizeof K, hipMemcpyHostToDevice, ctx().stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx().stream);                 // K is on this frame
        if (e != hipSuccess) { (void)hipFree(d); ZK_HIP(e); }
        g_pairing_consts[ci] = d;
    }
    *out = (const PairingConsts<C>*)g_pairing_consts[ci];
    return ZKMI_OK;
}

template <class C> int same_ratio_run(const uint8_t* g1s, const uint8_t* g1sx, const uint8_t* g2s, const uint8_t* g2sx, size_t n, int8_t* verdicts) {
    hipStream_t st = ctx().stream;
    const PairingConsts<C>* K;
    ZK_TRY(pairing_consts_dev<C>(&K));
    const size_t s1 = n * 2 * C::N * 4, s2 = 2 * s1;
    uint8_t* d;
    ZK_TRY(ws_get("p2v.same_ratio", 2 * s1 + 2 * s2 + n, (void**)&d));
    ZK_HIP(hipMemcpyAsync(d, g1s, s1, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d + s1, g1sx, s1, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d + 2 * s1, g2s, s2, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d + 2 * s1 + s2, g2sx, s2, hipMemcpyHostToDevice, st));
    ZK_HIP(hipEventRecord(ctx().ev0, st));
    hipLaunchKernelGGL(k_same_ratio<C>, dim3((unsigned)((n + SR_BLOCK - 1) / SR_BLOCK)), dim3(SR_BLOCK), 0, st, (const uint32_t*)d, (const uint32_t*)(d + s1),
                       (const uint32_t*)(d + 2 * s1), (const uint32_t*)(d + 2 * s1 + s2), (uint64_t)n, K, (int8_t*)(d + 2 * s1 + 2 * s2));
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipEventRecord(ctx().ev1, st));
    ZK_HIP(hipMemcpyAsync(verdicts, d + 2 * s1 + 2 * s2, n, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    return ZKMI_OK;
}

// ---- the generator -----------------------------------------------------------------------------------------------------------------------------------
chacha::Seed seed_of(const uint32_t* seed8) { chacha::Seed s; memcpy(s.w, seed8, 32); return s; }

int chacha_words_run(const uint32_t* seed8, uint64_t first_word, void* d_out, size_t n_words) {
    if (!n_words) return ZKMI_OK;
    if (first_word + n_words < first_word || n_words > ((size_t)1 << 40)) return fail(ZKMI_ERR_UNSUPPORTED, "chacha_words_dev: at most 2^40 words, below word 2^64");
    const uint64_t blocks = (first_word % 16 + n_words + 15) / 16;
    hipLaunchKernelGGL(chacha::k_chacha_words, dim3((unsigned)((blocks + chacha::T - 1) / chacha::T)), dim3(chacha::T), 0, ctx().stream, seed_of(seed8), first_word, (uint32_t*)d_out,
                       (uint64_t)n_words);
    ZK_HIP(hipGetLastError());
    return ZKMI_OK;
}

size_t g_round_blocks = 0;                         // zkmi_chacha_set_round_blocks: blocks per round (0: by the keep rate)

// Rounds of count, scan and scatter until n attempts are kept. A round takes as many blocks as the keep rate of the curve (r / 2^bits: 0.756 / 0.906)
// predicts for what is missing, plus 1 / 32 and 16 blocks; what a round keeps goes behind what the rounds before it kept, so the places do not depend on
// where the rounds are cut.
template <class FrC> int chacha_fr_run(const uint32_t* seed8, void* d_out, size_t n, uint64_t* words_consumed) {
    hipStream_t st = ctx().stream;
    if (words_consumed) *words_consumed = 0;
    if (!n) return ZKMI_OK;
    if (n > ((size_t)1 << 32)) return fail(ZKMI_ERR_UNSUPPORTED, "chacha_fr_dev: at most 2^32 elements");
    const chacha::Seed seed = seed_of(seed8);
    constexpr int bits = chacha::modulus_bits<FrC>();
    const double rate = (double)FrC::p(7) / (double)(1ull << (bits - 224));
    uint64_t *d_last, h_last = 0;
    uint32_t* d_total;
    ZK_TRY(ws_get("p2v.chacha_last", 16, (void**)&d_last));
    d_total = (uint32_t*)(d_last + 1);
    uint64_t kept = 0, first_block = 0;
    while (kept < n) {
        const uint64_t need = n - kept;
        uint64_t nb = g_round_blocks ? g_round_blocks : (uint64_t)((double)need / (2.0 * rate) * (1.0 + 1.0 / 32)) + 16;
        if (nb > ((uint64_t)1 << 30)) nb = (uint64_t)1 << 30;
        const uint32_t n_wg = (uint32_t)((nb + chacha::T - 1) / chacha::T);
        uint32_t *d_wg, total = 0;
        ZK_TRY(ws_get("p2v.chacha_wg", (size_t)n_wg * 4, (void**)&d_wg));
        hipLaunchKernelGGL((chacha::k_chacha_fr_count<FrC>), dim3(n_wg), dim3(chacha::T), 0, st, seed, first_block, (uint32_t)nb, d_wg);
        hipLaunchKernelGGL(chacha::k_chacha_scan, dim3(1), dim3(chacha::T), 0, st, d_wg, n_wg, d_total);
        hipLaunchKernelGGL((chacha::k_chacha_fr_scatter<FrC>), dim3(n_wg), dim3(chacha::T), 0, st, seed, first_block, (uint32_t)nb, (const uint32_t*)d_wg, kept, (uint64_t)n,
                           (uint32_t*)d_out, d_last);
        ZK_HIP(hipGetLastError());
        ZK_HIP(hipMemcpyAsync(&total, d_total, 4, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipStreamSynchronize(st));
        kept += total;
        first_block += nb;
    }
    ZK_HIP(hipMemcpyAsync(&h_last, d_last, 8, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    if (words_consumed) *words_consumed = 8 * (h_last + 1);
    return ZKMI_OK;
}
int chacha_fr_dispatch(int curve, const uint32_t* seed8, void* d_out, size_t n, uint64_t* words_consumed) {
    return curve == ZKMI_CURVE_BN128 ? chacha_fr_run<Bn254Fr>(seed8, d_out, n, words_consumed) : chacha_fr_run<Bls12381Fr>(seed8, d_out, n, words_consumed);
}

// ---- the two sums of a section check --------------------------------------------------------------------------------------------------------------------
int ratio_check(const char* who, int curve, const uint32_t* seed8, const uint8_t* o1, const uint8_t* o2) {
    if (curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) return fail(ZKMI_ERR_INVALID, std::string(who) + ": unknown curve");
    if (!seed8 || !o1 || !o2) return fail(ZKMI_ERR_INVALID, std::string(who) + ": null argument");
    if (pipeline_busy()) return fail(ZKMI_ERR_INVALID, std::string(who) + ": a pipeline slot holds work in flight (collect it first)");
    return ZKMI_OK;
}

int section_ratio_run(int curve, const zkmi_pages& a, const zkmi_pages& b, size_t n, const uint32_t* seed8, uint8_t* out_a, uint8_t* out_b) {
    const size_t sG1 = 2 * (size_t)n8q_of(curve);
    DevMem dm("phase2_section_ratio");
    void *d_pts, *d_s;
    ZK_TRY(dm.get(n * sG1, &d_pts));
    ZK_TRY(dm.get(n * 4, &d_s));
    ZK_TRY(chacha_words_run(seed8, 0, d_s, n));
    ZK_TRY(upload_pages(a, n * sG1, d_pts));
    ZK_TRY(zkmi_msm_dev(curve, 1, d_pts, d_s, n, 4, out_a));
    ZK_TRY(upload_pages(b, n * sG1, d_pts));
    ZK_TRY(zkmi_msm_dev(curve, 1, d_pts, d_s, n, 4, out_b));
    ZK_HIP(hipStreamSynchronize(ctx().stream));
    return ZKMI_OK;
}

template <class FqC, class FrC> int h_ratio_run(int curve, const zkmi_pages& tau_g1, const zkmi_pages& h, uint32_t power, const uint32_t* seed8, uint8_t* out_r1, uint8_t* out_r2) {
    typedef Fp<FqC> F1;
    constexpr size_t sG1 = 2 * FqC::N * 4;
    hipStream_t st = ctx().stream;
    const size_t dom = (size_t)1 << power;
    const uint32_t n = (uint32_t)(dom - 1);                                        // the term dom - 1 has scalar zero: tau[2 dom - 1] is never read
    DevMem dm("phase2_h_ratio");
    uint8_t *d_raw, *d_work;
    uint32_t *d_tau, *d_x, *d_pts;
    ZK_TRY(dm.get(dom * 32, (void**)&d_raw));
    ZK_TRY(dm.get(dom * 32, (void**)&d_work));
    ZK_TRY(dm.get((2 * dom - 1) * sG1, (void**)&d_tau));
    ZK_TRY(dm.get((size_t)n * 2 * sG1, (void**)&d_x));
    ZK_TRY(dm.get(dom * sG1, (void**)&d_pts));
    ZK_TRY(upload_pages(tau_g1, (2 * dom - 1) * sG1, d_tau));
    ZK_HIP(hipMemsetAsync(d_raw + (dom - 1) * 32, 0, 32, st));
    ZK_TRY(chacha_fr_dispatch(curve, seed8, d_raw, n, nullptr));
    // R1 = sum fromMontgomery(raw_i) (tau[dom + i] - tau[i])
    ZK_TRY(fr_batch_dev_dispatch(curve, ZKMI_BATCH_FROM_MONTGOMERY, d_raw, d_work, n));
    hipLaunchKernelGGL((k_setup_hdiff<F1>), dim3((n + 255) / 256), dim3(256), 0, st, d_tau, d_x, n, (uint32_t)dom);
    hipLaunchKernelGGL((k_setup_affine<F1>), dim3(((n + SETUP_INV - 1) / SETUP_INV + 255) / 256), dim3(256), 0, st, d_x, d_pts, n);
    ZK_HIP(hipGetLastError());
    ZK_TRY(zkmi_msm_dev(curve, 1, d_pts, d_work, n, 32, out_r1));
    // R2 = sum t_i H_i, t = fromMontgomery(fft(applyKey(raw, -2, w[power + 1])))
    const host::HField<4> Fr = host::HField<4>::from_cfg<FrC>();
    const host::HFp<4> first = Fr.neg(Fr.from_u64(2));
    uint8_t inc[32];
    ZK_TRY(fr_root(curve, power + 1, inc));
    ZK_TRY(ntt_dev_dispatch(curve, d_raw, d_work, power, 0, (const uint8_t*)first.v, inc));
    ZK_TRY(fr_batch_dev_dispatch(curve, ZKMI_BATCH_FROM_MONTGOMERY, d_work, d_raw, dom));
    ZK_TRY(upload_pages(h, dom * sG1, d_pts));
    ZK_TRY(zkmi_msm_dev(curve, 1, d_pts, d_raw, dom, 32, out_r2));
    ZK_HIP(hipStreamSynchronize(st));
    return ZKMI_OK;
}

int fr_s(int curve) { return curve == ZKMI_CURVE_BN128 ? 28 : 32; }

// ---- the host restatements the tests hold the kernels to --------------------------------------------------------------------------------------------
template <class FrC> uint64_t fr_sequential_host(const uint32_t* seed8, uint8_t* out, size_t n) {
    const host::HField<4> Fr = host::HField<4>::from_cfg<FrC>();
    phase2::ChaCha rng(seed8);
    uint64_t blocks = 0;
    for (size_t i = 0; i < n; i++) {
        const host::HFp<4> v = phase2::field_from_rng(Fr, rng);
        memcpy(out + 32 * i, v.v, 32);
    }
    if (!n) return 0;
    // the position: blocks drawn so far (the struct's counter has no borrow here: fewer than 2^32 blocks) less what is left of the last one
    blocks = ((uint64_t)rng.state[13] << 32) | rng.state[12];
    return 16 * blocks - (16 - (uint64_t)rng.idx);
}

}  // namespace
}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zkmi_chacha_words_dev(const uint32_t* seed8, uint64_t first_word, void* d_out, size_t n_words) {
    ZK_TRY(require_ctx());
    if (!seed8 || (n_words && !d_out)) return fail(ZKMI_ERR_INVALID, "chacha_words_dev: null argument");
    return chacha_words_run(seed8, first_word, d_out, n_words);
}

int zkmi_chacha_fr_dev(int curve, const uint32_t* seed8, void* d_out, size_t n, uint64_t* words_consumed) {
    ZK_TRY(require_ctx());
    if (curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) return fail(ZKMI_ERR_INVALID, "chacha_fr_dev: unknown curve");
    if (!seed8 || (n && !d_out)) return fail(ZKMI_ERR_INVALID, "chacha_fr_dev: null argument");
    if ((uintptr_t)d_out & 15) return fail(ZKMI_ERR_INVALID, "chacha_fr_dev: the output must be 16-byte aligned");
    return chacha_fr_dispatch(curve, seed8, d_out, n, words_consumed);
}

int zkmi_same_ratio_batch(int curve, const uint8_t* g1s, const uint8_t* g1sx, const uint8_t* g2s, const uint8_t* g2sx, size_t n, int8_t* verdicts) {
    ZK_TRY(require_ctx());
    if (curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) return fail(ZKMI_ERR_INVALID, "same_ratio_batch: unknown curve");
    if (!n) return ZKMI_OK;
    if (!g1s || !g1sx || !g2s || !g2sx || !verdicts) return fail(ZKMI_ERR_INVALID, "same_ratio_batch: null argument");
    if (n > ((size_t)1 << 24)) return fail(ZKMI_ERR_UNSUPPORTED, "same_ratio_batch: at most 2^24 checks");
    return curve == ZKMI_CURVE_BN128 ? same_ratio_run<Bn254Fq>(g1s, g1sx, g2s, g2sx, n, verdicts) : same_ratio_run<Bls12381Fq>(g1s, g1sx, g2s, g2sx, n, verdicts);
}

int zkmi_phase2_section_ratio(int curve, zkmi_pages a, zkmi_pages b, size_t n, const uint32_t* seed8, uint8_t* out_a, uint8_t* out_b) {
    ZK_TRY(require_ctx());
    ZK_TRY(ratio_check("phase2_section_ratio", curve, seed8, out_a, out_b));
    if (n >= ((size_t)1 << 31)) return fail(ZKMI_ERR_UNSUPPORTED, "phase2_section_ratio: at most 2^31 - 1 points");
    const size_t bytes = n * 2 * n8q_of(curve);
    if (pages_bytes(a) < bytes || pages_bytes(b) < bytes) return fail(ZKMI_ERR_INVALID, "phase2_section_ratio: a section is shorter than n points");
    memset(out_a, 0, 3 * n8q_of(curve));
    memset(out_b, 0, 3 * n8q_of(curve));
    if (!n) return ZKMI_OK;
    return section_ratio_run(curve, a, b, n, seed8, out_a, out_b);
}

int zkmi_phase2_h_ratio(int curve, zkmi_pages tau_g1, zkmi_pages h, uint32_t power, const uint32_t* seed8, uint8_t* out_r1, uint8_t* out_r2) {
    ZK_TRY(require_ctx());
    ZK_TRY(ratio_check("phase2_h_ratio", curve, seed8, out_r1, out_r2));
    if ((int)power >= fr_s(curve)) return fail(ZKMI_ERR_UNSUPPORTED, "phase2_h_ratio: power >= Fr.s takes the reference's other branch (coset shift), which is not built");
    if (power < 1) return fail(ZKMI_ERR_INVALID, "phase2_h_ratio: domainSize must be at least 2");
    const size_t dom = (size_t)1 << power, sG1 = 2 * (size_t)n8q_of(curve);
    if (pages_bytes(tau_g1) < (2 * dom - 1) * sG1) return fail(ZKMI_ERR_INVALID, "phase2_h_ratio: the tauG1 slice must hold 2 domainSize - 1 points");
    if (pages_bytes(h) < dom * sG1) return fail(ZKMI_ERR_INVALID, "phase2_h_ratio: the H section must hold domainSize points");
    return curve == ZKMI_CURVE_BN128 ? h_ratio_run<Bn254Fq, Bn254Fr>(curve, tau_g1, h, power, seed8, out_r1, out_r2)
                                     : h_ratio_run<Bls12381Fq, Bls12381Fr>(curve, tau_g1, h, power, seed8, out_r1, out_r2);
}

// ---- diagnostics (include/zkmi_diag.h): host only ---------------------------------------------------------------------------------------------------
int zkmi_chacha_block_host(const uint32_t* seed8, uint64_t counter_lo, uint64_t counter_hi, uint32_t* out16) {
    if (!seed8 || !out16) return fail(ZKMI_ERR_INVALID, "chacha_block_host: null argument");
    chacha::block(seed8, counter_lo, counter_hi, out16);
    return ZKMI_OK;
}
int zkmi_chacha_struct_words_host(const uint32_t* seed8, uint64_t first_word, uint32_t* out, size_t n_words) {
    if (!seed8 || (n_words && !out)) return fail(ZKMI_ERR_INVALID, "chacha_struct_words_host: null argument");
    phase2::ChaCha rng(seed8);
    const uint64_t b = first_word / 16;
    rng.state[12] = (uint32_t)b; rng.state[13] = (uint32_t)(b >> 32);
    for (uint64_t k = 0; k < first_word % 16; k++) (void)rng.next_u32();
    for (size_t j = 0; j < n_words; j++) out[j] = rng.next_u32();
    return ZKMI_OK;
}
int zkmi_chacha_fr_host(int curve, const uint32_t* seed8, uint8_t* out, size_t n, uint64_t* words_consumed) {
    if ((curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) || !seed8 || (n && !out)) return fail(ZKMI_ERR_INVALID, "chacha_fr_host: bad argument");
    const uint64_t w = curve == ZKMI_CURVE_BN128 ? fr_sequential_host<Bn254Fr>(seed8, out, n) : fr_sequential_host<Bls12381Fr>(seed8, out, n);
    if (words_consumed) *words_consumed = w;
    return ZKMI_OK;
}
int zkmi_chacha_fr_compact_host(int curve, const uint32_t* seed8, uint8_t* out, size_t n, uint64_t* words_consumed) {
    if ((curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) || !seed8 || (n && !out)) return fail(ZKMI_ERR_INVALID, "chacha_fr_compact_host: bad argument");
    const uint64_t w = curve == ZKMI_CURVE_BN128 ? chacha::fr_stream_host<Bn254Fr>(seed8, out, n) : chacha::fr_stream_host<Bls12381Fr>(seed8, out, n);
    if (words_consumed) *words_consumed = w;
    return ZKMI_OK;
}
int zkmi_chacha_set_round_blocks(size_t blocks) {
    if (blocks > ((size_t)1 << 30)) return fail(ZKMI_ERR_INVALID, "chacha_set_round_blocks: at most 2^30 blocks per round");
    g_round_blocks = blocks;
    return ZKMI_OK;
}

}  // extern "C"
