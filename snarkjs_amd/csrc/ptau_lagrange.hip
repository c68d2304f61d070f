// snarkjs_amd/csrc/ptau_lagrange.hip — host driver + C-ABI of the Lagrange ladder of powersOfTau.preparePhase2 / convert (ptau_lagrange.cuh).
#include <string.h>
#include "ptau_lagrange.cuh"
#include "host_field.hpp"
#include "setup_common.hpp"
#include "zkmi_common.hpp"

namespace zkmi {
namespace {

int lag_fr_s(int curve) { return curve == ZKMI_CURVE_BN128 ? 28 : 32; }

template <class F, class FrC> int lag_run(int curve, const void* d_tau, void* d_out, uint32_t first, uint32_t top, int zero_last) {
    constexpr int FW = FieldWords<F>::value;
    Ctx& cx = ctx();
    hipStream_t st = cx.stream;
    const size_t pts = lag_points(first, top);
    uint32_t *work, *d_inv2;
    ZK_TRY(ws_get("ptaulag.work", pts * 4 * FW * 4, (void**)&work));
    ZK_TRY(ws_get("ptaulag.inv2", (PTAU_LAG_MAX_TOP + 1) * 32, (void**)&d_inv2));
    // 2^-p, p = 0 .. top, in normal form: the store kernel reads them as plain scalars
    const host::HField<4> Fr = host::HField<4>::from_cfg<FrC>();
    uint64_t h_inv2[(PTAU_LAG_MAX_TOP + 1) * 4];
    const host::HFp<4> half = Fr.inv(Fr.from_u64(2));
    host::HFp<4> acc = Fr.One();
    for (uint32_t p = 0; p <= top; p++) {
        const host::HFp<4> nrm = Fr.from_mont(acc);
        memcpy(h_inv2 + 4 * p, nrm.v, 32);
        acc = Fr.mul(acc, half);
    }
    ZK_HIP(hipMemcpyAsync(d_inv2, h_inv2, (size_t)(top + 1) * 32, hipMemcpyHostToDevice, st));
    ZK_HIP(hipStreamSynchronize(st));                           // `h_inv2` is a stack buffer
    GfftTw tw{nullptr, nullptr, 0, top};
    const uint32_t* n_inv = nullptr;
    if (top) ZK_TRY(ntt_power_tables(curve, top, 1, &tw.T_lo, &tw.T_hi, &tw.log_lb, &n_inv));
    const unsigned pt_blocks = (unsigned)((pts + 255) / 256), bf_blocks = (unsigned)((((size_t)1 << top) + 255) / 256);
    ZK_HIP(hipEventRecord(cx.ev0, st));
    hipLaunchKernelGGL((k_ptau_lag_load<F>), dim3(pt_blocks), dim3(256), 0, st, (const uint32_t*)d_tau, work, first, top, zero_last);
    for (uint32_t s = 1; s <= top; s++) hipLaunchKernelGGL((k_ptau_lag_stage<F, FrC>), dim3(bf_blocks), dim3(256), 0, st, work, s, first, top, tw);
    hipLaunchKernelGGL((k_ptau_lag_store<F>), dim3(pt_blocks), dim3(256), 0, st, (const uint32_t*)work, (uint32_t*)d_out, first, top, (const uint32_t*)d_inv2);
    ZK_HIP(hipEventRecord(cx.ev1, st));
    ZK_HIP(hipGetLastError());
    return ZKMI_OK;
}
int lag_dispatch(int curve, int group, const void* d_tau, void* d_out, uint32_t first, uint32_t top, int zero_last) {
    if (curve == ZKMI_CURVE_BN128)
        return group == 1 ? lag_run<Fp<Bn254Fq>, Bn254Fr>(curve, d_tau, d_out, first, top, zero_last) : lag_run<Fp2<Bn254Fq>, Bn254Fr>(curve, d_tau, d_out, first, top, zero_last);
    return group == 1 ? lag_run<Fp<Bls12381Fq>, Bls12381Fr>(curve, d_tau, d_out, first, top, zero_last) : lag_run<Fp2<Bls12381Fq>, Bls12381Fr>(curve, d_tau, d_out, first, top, zero_last);
}
// everything both entry points check before anything is allocated
int lag_check(const char* who, int curve, int group, size_t n_tau, uint32_t first, uint32_t top, int zero_last) {
    const std::string w(who);
    if (curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) return fail(ZKMI_ERR_INVALID, w + ": unknown curve");
    if (group != 1 && group != 2) return fail(ZKMI_ERR_INVALID, w + ": group must be 1 or 2");
    if (pipeline_busy()) return fail(ZKMI_ERR_INVALID, w + ": a pipeline slot holds work in flight (collect it first)");
    if (top > (uint32_t)lag_fr_s(curve)) return fail(ZKMI_ERR_UNSUPPORTED, w + ": top > Fr.s (a transform of 2^top elements is beyond the 2-adicity of Fr)");
    if (top > PTAU_LAG_MAX_TOP) return fail(ZKMI_ERR_UNSUPPORTED, w + ": at most 2^28 points in the top block");
    if (first > top) return fail(ZKMI_ERR_INVALID, w + ": first > top");
    if (n_tau != ((size_t)1 << top) - (zero_last ? 1 : 0)) return fail(ZKMI_ERR_INVALID, w + ": the tau section must hold 2^top points (one fewer with zero_last)");
    return ZKMI_OK;
}

}  // namespace
}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zkmi_ptau_lagrange_dev(int curve, int group, const void* d_tau, size_t n_tau, void* d_out, uint32_t first, uint32_t top, int zero_last) {
    ZK_TRY(require_ctx());
    ZK_TRY(lag_check("ptau_lagrange_dev", curve, group, n_tau, first, top, zero_last));
    if ((n_tau && !d_tau) || !d_out) return fail(ZKMI_ERR_INVALID, "ptau_lagrange_dev: null buffer");
    return lag_dispatch(curve, group, d_tau, d_out, first, top, zero_last ? 1 : 0);
}

int zkmi_ptau_lagrange_section(int curve, int group, zkmi_pages tau, size_t n_tau, uint32_t first, uint32_t top, int zero_last, uint8_t* const* out_ptr, const size_t* out_len,
                               int n_out_pages) {
    ZK_TRY(require_ctx());
    ZK_TRY(lag_check("ptau_lagrange_section", curve, group, n_tau, first, top, zero_last));
    if (!out_ptr || !out_len) return fail(ZKMI_ERR_INVALID, "ptau_lagrange_section: null argument");
    const size_t sG = (size_t)2 * group * n8q_of(curve), in_bytes = n_tau * sG, out_bytes = (size_t)lag_points(first, top) * sG;
    if (pages_bytes(tau) < in_bytes) return fail(ZKMI_ERR_INVALID, "ptau_lagrange_section: the tau section is shorter than n_tau points");
    size_t cap = 0;
    for (int i = 0; i < n_out_pages; i++) cap += out_len[i];
    if (cap < out_bytes) return fail(ZKMI_ERR_INVALID, "ptau_lagrange_section: out is shorter than 2^(top + 1) - 2^first points");
    DevMem dm("ptau_lagrange_section");
    uint8_t *d_tau, *d_out;
    ZK_TRY(dm.get(in_bytes ? in_bytes : 1, (void**)&d_tau));
    ZK_TRY(dm.get(out_bytes, (void**)&d_out));
    if (in_bytes) ZK_TRY(upload_pages(tau, in_bytes, d_tau));
    ZK_TRY(lag_dispatch(curve, group, d_tau, d_out, first, top, zero_last ? 1 : 0));
    return download_pages(d_out, out_bytes, out_ptr, out_len, n_out_pages);
}

}  // extern "C"
