// snarkjs_amd/csrc/ptau_verify.hip — host driver + C-ABI of what powersOfTau.verify computes on one section of a .ptau (src/powersoftau_verify.js:
// processSection and verifyLagrangeEvaluations). One upload per section; the points are converted, summed and transformed by the kernels the
// library already has (zkmi_group_convert_dev, zkmi_chacha_words_dev, zkmi_msm_dev, zkmi_ntt_dev). The one kernel here widens the generator's 32-bit words
// into the 32-byte scalars the transform takes. Blake2b with a restorable state is in ptau_host.hpp.
#include <string.h>
#include <vector>
#include "field.cuh"
#include "host_field.hpp"
#include "ptau_host.hpp"
#include "setup_common.hpp"
#include "zkmi_common.hpp"

namespace zkmi {
namespace {

constexpr int WIDEN_BLOCK = 256;

// out[i] = w[i] as a 32-byte little-endian element, one element per lane in two 16-byte stores; zero_last: element n - 1 is zero and w[n - 1] is not read
__global__ void __launch_bounds__(WIDEN_BLOCK) k_ptau_widen(const uint32_t* __restrict__ w, uint4* __restrict__ out, uint64_t n, int zero_last) {
    const uint64_t i = (uint64_t)blockIdx.x * WIDEN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = (zero_last && i == n - 1) ? 0u : w[i];
    out[2 * i] = make_uint4(v, 0u, 0u, 0u);
    out[2 * i + 1] = make_uint4(0u, 0u, 0u, 0u);
}

int fr_s(int curve) { return curve == ZKMI_CURVE_BN128 ? 28 : 32; }

template <class FT> bool eq_bytes(const host::HCurve<FT>& G, const uint8_t* a, const uint8_t* b) {
    host::HPoint<FT> pa, pb;
    static_assert(sizeof pa == 3 * sizeof(typename FT::E), "a Jacobian point is three packed elements");
    memcpy(&pa, a, sizeof pa); memcpy(&pb, b, sizeof pb);
    return ptau::jacobian_eq(G, pa, pb);
}
template <class FqC> bool jac_eq_curve(int group, const uint8_t* a, const uint8_t* b) {
    constexpr int L = FqC::N / 2;
    const host::HField<L> F = host::HField<L>::template from_cfg<FqC>();
    if (group == 1) return eq_bytes(host::HCurve<host::HField<L>>{F}, a, b);
    return eq_bytes(host::HCurve<host::HField2<L>>{host::HField2<L>{F}}, a, b);
}
bool jac_eq(int curve, int group, const uint8_t* a, const uint8_t* b) {
    return curve == ZKMI_CURVE_BN128 ? jac_eq_curve<Bn254Fq>(group, a, b) : jac_eq_curve<Bls12381Fq>(group, a, b);
}

struct SectionArgs {
    int curve, group;
    const zkmi_pages* tau;
    size_t n_tau;
    const zkmi_pages* lagrange;
    uint32_t top;
    int zero_last;
    const uint32_t *pair_seed, *ladder_seed;
    uint8_t* const* u_ptr;
    const size_t* u_len;
    int n_u_pages;
    uint8_t *r1, *r2;
    int8_t* ladder;
};

int section_check_run(const SectionArgs& a) {
    const int curve = a.curve, group = a.group;
    const size_t sG = (size_t)2 * group * n8q_of(curve), jac = (size_t)3 * group * n8q_of(curve);
    const size_t N = (size_t)1 << a.top, n = a.n_tau;
    hipStream_t st = ctx().stream;
    DevMem dm("ptau_section_check");
    uint8_t *d_tau, *d_u, *d_lag = nullptr, *d_wide = nullptr, *d_fft = nullptr;
    uint32_t* d_words;
    ZK_TRY(dm.get(n * sG, (void**)&d_tau));
    ZK_TRY(dm.get(n * sG, (void**)&d_u));
    ZK_TRY(dm.get((a.lagrange ? std::max(n, N) : n) * 4, (void**)&d_words));
    if (n) {
        ZK_TRY(upload_pages(*a.tau, n * sG, d_tau));
        ZK_TRY(zkmi_group_convert_dev(curve, group, ZKMI_CONV_LEM_TO_U, d_tau, d_u, n));
        ZK_TRY(download_pages(d_u, n * sG, a.u_ptr, a.u_len, a.n_u_pages));
    }
    // the two sums of processSection: one set of scalars, the section at offsets of 0 and one point
    if (n > 1) {
        ZK_TRY(zkmi_chacha_words_dev(a.pair_seed, 0, d_words, n - 1));
        ZK_TRY(zkmi_msm_dev(curve, group, d_tau, d_words, n - 1, 4, a.r1));
        ZK_TRY(zkmi_msm_dev(curve, group, d_tau + sG, d_words, n - 1, 4, a.r2));
    }
    if (!a.lagrange) { ZK_HIP(hipStreamSynchronize(st)); return ZKMI_OK; }
    // verifyLagrangeEvaluations: the generator is restarted for every power, so the words of power p are a prefix of those of p + 1
    ZK_TRY(dm.get((2 * N - 1) * sG, (void**)&d_lag));
    ZK_TRY(dm.get(N * 32, (void**)&d_wide));
    ZK_TRY(dm.get(N * 32, (void**)&d_fft));
    ZK_TRY(upload_pages(*a.lagrange, (2 * N - 1) * sG, d_lag));
    ZK_TRY(zkmi_chacha_words_dev(a.ladder_seed, 0, d_words, N));
    hipLaunchKernelGGL(k_ptau_widen, dim3((unsigned)((N + WIDEN_BLOCK - 1) / WIDEN_BLOCK)), dim3(WIDEN_BLOCK), 0, st, (const uint32_t*)d_words, (uint4*)d_wide, (uint64_t)N, a.zero_last);
    ZK_HIP(hipGetLastError());
    std::vector<uint8_t> left(jac, 0), seg(jac), right(jac);
    for (uint32_t p = 0; p <= a.top; p++) {
        // left side: the running sum over the dyadic segments [0, 1), [1, 2), [2, 4), ..; the last term of the top power has scalar zero when zero_last
        const size_t first = p ? (size_t)1 << (p - 1) : 0, end = ((size_t)1 << p) - ((p == a.top && a.zero_last) ? 1 : 0);
        if (end > first) {
            ZK_TRY(zkmi_msm_dev(curve, group, d_tau + first * sG, d_words + first, end - first, 4, seg.data()));
            ZK_TRY(zkmi_point_add(curve, group, left.data(), seg.data(), left.data()));
        }
        // right side: the transform of the widened prefix against the block of 2^p Lagrange points
        ZK_TRY(zkmi_ntt_dev(curve, d_wide, d_fft, p, 0, nullptr, nullptr));
        ZK_TRY(zkmi_msm_dev(curve, group, d_lag + (((size_t)1 << p) - 1) * sG, d_fft, (size_t)1 << p, 32, right.data()));
        a.ladder[p] = jac_eq(curve, group, left.data(), right.data()) ? 1 : 0;
    }
    ZK_HIP(hipStreamSynchronize(st));
    return ZKMI_OK;
}

}  // namespace
}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zkmi_ptau_section_check(int curve, int group, zkmi_pages tau, size_t n_tau, const zkmi_pages* lagrange, uint32_t top, int zero_last, const uint32_t* pair_seed8,
                            const uint32_t* ladder_seed8, uint8_t* const* u_out_ptr, const size_t* u_out_len, int n_u_pages, uint8_t* r1, uint8_t* r2, int8_t* ladder) {
    ZK_TRY(require_ctx());
    if (curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) return fail(ZKMI_ERR_INVALID, "ptau_section_check: unknown curve");
    if (group != 1 && group != 2) return fail(ZKMI_ERR_INVALID, "ptau_section_check: group must be 1 or 2");
    if (!pair_seed8 || !r1 || !r2 || (lagrange && (!ladder_seed8 || !ladder)) || (n_tau && (!u_out_ptr || !u_out_len))) return fail(ZKMI_ERR_INVALID, "ptau_section_check: null argument");
    if (pipeline_busy()) return fail(ZKMI_ERR_INVALID, "ptau_section_check: a pipeline slot holds work in flight (collect it first)");
    if (n_tau >= ((size_t)1 << 31)) return fail(ZKMI_ERR_UNSUPPORTED, "ptau_section_check: at most 2^31 - 1 points");
    const size_t sG = (size_t)2 * group * n8q_of(curve);
    if (pages_bytes(tau) < n_tau * sG) return fail(ZKMI_ERR_INVALID, "ptau_section_check: the tau section is shorter than n_tau points");
    size_t cap = 0;
    for (int i = 0; i < n_u_pages && n_tau; i++) cap += u_out_len[i];
    if (cap < n_tau * sG) return fail(ZKMI_ERR_INVALID, "ptau_section_check: u_out is shorter than n_tau points");
    if (top > (uint32_t)fr_s(curve)) return fail(ZKMI_ERR_UNSUPPORTED, "ptau_section_check: top > Fr.s (a transform of 2^top elements is beyond the 2-adicity of Fr)");
    if (lagrange) {
        const size_t N = (size_t)1 << top;
        if (n_tau < N - (zero_last ? 1 : 0)) return fail(ZKMI_ERR_INVALID, "ptau_section_check: the tau section must hold 2^top points (one fewer with zero_last)");
        if (pages_bytes(*lagrange) < (2 * N - 1) * sG) return fail(ZKMI_ERR_INVALID, "ptau_section_check: the Lagrange section must hold 2^(top + 1) - 1 points");
    }
    memset(r1, 0, 3 * (size_t)group * n8q_of(curve));
    memset(r2, 0, 3 * (size_t)group * n8q_of(curve));
    const SectionArgs a{curve, group, &tau, n_tau, lagrange, top, zero_last ? 1 : 0, pair_seed8, ladder_seed8, u_out_ptr, u_out_len, n_u_pages, r1, r2, ladder};
    return section_check_run(a);
}

int zkmi_blake2b512_resume(const uint8_t* partial216, const uint8_t* data, size_t len, uint8_t* out64) {
    if (!partial216 || !out64 || (len && !data)) return fail(ZKMI_ERR_INVALID, "blake2b512_resume: null argument");
    ptau::Blake2b512 hs;
    if (!hs.restore(partial216)) return fail(ZKMI_ERR_INVALID, "blake2b512_resume: the position lies beyond the 128-byte block buffer");
    hs.update(data, len);
    hs.digest(out64);
    return ZKMI_OK;
}

}  // extern "C"
