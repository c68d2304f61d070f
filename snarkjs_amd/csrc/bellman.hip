// snarkjs_amd/csrc/bellman.hip — host driver + C-ABI of the H basis change of zKey.exportBellman / zKey.importBellman (bellman.cuh): section 9
// of a Groth16 key to the H points of a Bellman-format parameter file and back, from one upload to one download.
#include <string.h>
#include "bellman.cuh"
#include "gfft.cuh"
#include "host_field.hpp"
#include "setup_common.hpp"
#include "zkmi_common.hpp"

namespace zkmi {
namespace {

int fr_s(int curve) { return curve == ZKMI_CURVE_BN128 ? 28 : 32; }

// R'^2 mod p as canonical words: 2^(2 B NL), out of the host field's Montgomery form
template <class C, int HL> BellmanRR<C::N> rr_of() {
    const host::HField<HL> Fq = host::HField<HL>::template from_cfg<C>();
    const host::HFp<HL> v = Fq.from_mont(Fq.pow_u64(Fq.from_u64(2), (uint64_t)2 * Lim29<C>::B * Lim29<C>::NL));
    BellmanRR<C::N> rr;
    memcpy(rr.w, v.v, sizeof rr.w);
    return rr;
}

// C: the base field as the new kernels see it (the 14-limb curve with called products, as k_group_mul_each runs it and for its reason); Cb: the same field
// without the wrapper, for the stage kernel and the host arithmetic
template <class C, class Cb, class FrC, int HL> int h_section_run(int curve, const void* d_in, void* d_out, unsigned L, int direction) {
    typedef Fp<Cb> F;
    constexpr int N = Cb::N;
    Ctx& cx = ctx();
    hipStream_t st = cx.stream;
    const uint32_t n = 1u << L;
    const host::HField<4> Fr = host::HField<4>::from_cfg<FrC>();
    // export: -2 w^i; import: -(2 n)^-1 w^-i; w = Fr.w[L + 1]
    host::HFp<4> w;
    ZK_TRY(fr_root(curve, L + 1, (uint8_t*)w.v));
    host::HFp<4> first = Fr.neg(Fr.from_u64(2)), inc = w;
    if (direction) { first = Fr.neg(Fr.inv(Fr.from_u64((uint64_t)2 * n))); inc = Fr.inv(w); }
    const host::HFp<4> inc256 = Fr.pow_u64(inc, 256);
    uint32_t *work, *d_scal, *d_k;
    ZK_TRY(ws_get("bellman.work", (size_t)n * 4 * N * 4, (void**)&work));
    ZK_TRY(ws_get("bellman.scalars", (size_t)n * 32, (void**)&d_scal));
    ZK_TRY(ws_get("bellman.consts", 96, (void**)&d_k));
    uint8_t h[96];
    memcpy(h, first.v, 32); memcpy(h + 32, inc.v, 32); memcpy(h + 64, inc256.v, 32);
    ZK_HIP(hipMemcpyAsync(d_k, h, 96, hipMemcpyHostToDevice, st));
    ZK_HIP(hipStreamSynchronize(st));                           // `h` is a stack buffer
    GfftTw tw{nullptr, nullptr, 0, L};
    const uint32_t* n_inv = nullptr;
    ZK_TRY(ntt_power_tables(curve, L, direction, &tw.T_lo, &tw.T_hi, &tw.log_lb, &n_inv));
    const unsigned blocks = (n + 255) / 256, m = n - 1;
    ZK_HIP(hipEventRecord(cx.ev0, st));
    hipLaunchKernelGGL((k_bellman_scalars<FrC>), dim3((m + 255) / 256), dim3(256), 0, st, d_scal, m, d_k);
    if (direction) hipLaunchKernelGGL((k_bellman_import_load<C>), dim3(blocks), dim3(256), 0, st, (const uint32_t*)d_in, d_scal, work, n, L, (rr_of<Cb, HL>()));
    else hipLaunchKernelGGL((k_gfft_load<F>), dim3(blocks), dim3(256), 0, st, (const uint32_t*)d_in, work, n, L);
    for (unsigned s = 1; s <= L; s++) hipLaunchKernelGGL((k_gfft_stage<F, FrC>), dim3((n / 2 + 255) / 256), dim3(256), 0, st, work, n, s, tw);
    if (direction) hipLaunchKernelGGL((k_gfft_store<F, FrC>), dim3(blocks), dim3(256), 0, st, work, (uint32_t*)d_out, n, (const uint32_t*)nullptr);
    else {
        hipLaunchKernelGGL((k_bellman_export_twist<C>), dim3((m + 255) / 256), dim3(256), 0, st, work, d_scal, m);
        hipLaunchKernelGGL((k_bellman_export_store<C>), dim3(((m + SCALE_INV - 1) / SCALE_INV + 255) / 256), dim3(256), 0, st, work, (uint32_t*)d_out, m);
    }
    ZK_HIP(hipEventRecord(cx.ev1, st));
    ZK_HIP(hipGetLastError());
    return ZKMI_OK;
}

int h_section_dispatch(int curve, const void* d_in, void* d_out, unsigned L, int direction) {
    return curve == ZKMI_CURVE_BN128 ? h_section_run<Bn254Fq, Bn254Fq, Bn254Fr, 4>(curve, d_in, d_out, L, direction)
                                     : h_section_run<Compact<Bls12381Fq>, Bls12381Fq, Bls12381Fr, 6>(curve, d_in, d_out, L, direction);
}

int h_section_args(const char* who, int curve, unsigned log_n, int direction) {
    if ((curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) || (direction != 0 && direction != 1)) return fail(ZKMI_ERR_INVALID, std::string(who) + ": unknown curve or direction");
    if (log_n < 1) return fail(ZKMI_ERR_UNSUPPORTED, std::string(who) + ": domainSize must be at least 2");
    if (log_n + 1 > (unsigned)fr_s(curve)) return fail(ZKMI_ERR_UNSUPPORTED, std::string(who) + ": Fr.w[log_n + 1] is beyond the 2-adicity of Fr");
    if (log_n > 28) return fail(ZKMI_ERR_UNSUPPORTED, std::string(who) + ": at most 2^28 points (the group fft's bound)");      // BLS12-381 alone: Fr.s of BN254 stops at 27
    if (pipeline_busy()) return fail(ZKMI_ERR_INVALID, std::string(who) + ": a pipeline slot holds work in flight (collect it first)");
    return ZKMI_OK;
}

}  // namespace
}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zkmi_bellman_h_section_dev(int curve, const void* d_in, void* d_out, unsigned log_n, int direction) {
    static const char* const who = "bellman_h_section";
    ZK_TRY(require_ctx());
    ZK_TRY(h_section_args(who, curve, log_n, direction));
    if (!d_in || !d_out) return fail(ZKMI_ERR_INVALID, "bellman_h_section: null buffer");
    return h_section_dispatch(curve, d_in, d_out, log_n, direction);
}

int zkmi_bellman_h_section(int curve, zkmi_pages in, unsigned log_n, int direction, uint8_t* const* out_ptr, const size_t* out_len, int n_out_pages) {
    static const char* const who = "bellman_h_section";
    ZK_TRY(require_ctx());
    ZK_TRY(h_section_args(who, curve, log_n, direction));
    const size_t sG1 = (size_t)2 * n8q_of(curve), n = (size_t)1 << log_n;
    const size_t in_bytes = (direction ? n - 1 : n) * sG1, out_bytes = (direction ? n : n - 1) * sG1;
    if (!in.ptr || !in.len || !out_ptr || !out_len || n_out_pages < 0) return fail(ZKMI_ERR_INVALID, "bellman_h_section: null argument");
    if (pages_bytes(in) != in_bytes) return fail(ZKMI_ERR_INVALID, "bellman_h_section: the input pages do not hold the section's points");
    size_t cap = 0;
    for (int i = 0; i < n_out_pages; i++) {
        if (out_len[i] && !out_ptr[i]) return fail(ZKMI_ERR_INVALID, "bellman_h_section: null argument");
        cap += out_len[i];
    }
    if (cap != out_bytes) return fail(ZKMI_ERR_INVALID, "bellman_h_section: the output pages do not hold the section's points");
    DevMem dm(who);
    void *d_in, *d_out;
    ZK_TRY(dm.get(in_bytes, &d_in));
    ZK_TRY(dm.get(out_bytes, &d_out));
    ZK_TRY(upload_pages(in, in_bytes, d_in));
    ZK_TRY(h_section_dispatch(curve, d_in, d_out, log_n, direction));
    return download_pages(d_out, out_bytes, out_ptr, out_len, n_out_pages);
}

}  // extern "C"
