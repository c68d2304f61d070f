// snarkjs_amd/csrc/group_scale.hip — host driver + C-ABI of the one-scalar point scaling (group_scale.cuh) and the host-only helpers of a Groth16
// phase-2 contribution (phase2_host.hpp).
#include <string.h>
#include "group_scale.cuh"
#include "host_field.hpp"
#include "phase2_host.hpp"
#include "zkmi_common.hpp"

namespace zkmi {

template <class FrC> static ScaleDigits digits_of(const uint8_t* k_mont) {
    const host::HField<4> Fr = host::HField<4>::from_cfg<FrC>();
    host::HFp<4> k;
    memcpy(k.v, k_mont, 32);
    return scale_recode(Fr.from_mont(k).v);
}
static ScaleDigits digits_of(int curve, const uint8_t* k_mont) { return curve == ZKMI_CURVE_BN128 ? digits_of<Bn254Fr>(k_mont) : digits_of<Bls12381Fr>(k_mont); }

// phase 2 scales a single G2 point: group 2 goes to the general kernel with first = k, inc = 1
static host::HFp<4> fr_one(int curve) { return curve == ZKMI_CURVE_BN128 ? host::HField<4>::from_cfg<Bn254Fr>().One() : host::HField<4>::from_cfg<Bls12381Fr>().One(); }

// C: the base field as the kernels see it. The 14-limb curve runs with CALLED products (Compact, field29.cuh): a doubling and a mixed addition inlined
// are some 90 KB of straight-line code in one loop, more than the instruction cache holds
template <class C> static int group_scale_g1_run(const void* d_in, void* d_out, size_t n, const ScaleDigits& d) {
    Ctx& cx = ctx();
    uint32_t* work;
    ZK_TRY(ws_get("gscale.work", n * 4 * C::N * 4, (void**)&work));
    ZK_HIP(hipEventRecord(cx.ev0, cx.stream));
    hipLaunchKernelGGL((k_group_scale<C>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, cx.stream, (const uint32_t*)d_in, work, (uint32_t)n, d);
    const size_t groups = (n + SCALE_INV - 1) / SCALE_INV;
    hipLaunchKernelGGL((k_group_scale_affine<C>), dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, cx.stream, work, (uint32_t*)d_out, (uint32_t)n);
    ZK_HIP(hipEventRecord(cx.ev1, cx.stream));
    ZK_HIP(hipGetLastError());
    return ZKMI_OK;
}
static int group_scale_dispatch(int curve, int group, const void* d_in, void* d_out, size_t n, const uint8_t* k_mont) {
    if (!n) return ZKMI_OK;
    if (n >= (1ull << 31)) return fail(ZKMI_ERR_UNSUPPORTED, "group scale: at most 2^31 - 1 points");
    if (group == 2) return zkmi_group_batch_apply_key_dev(curve, 2, d_in, d_out, n, k_mont, (const uint8_t*)fr_one(curve).v);
    const ScaleDigits d = digits_of(curve, k_mont);
    return curve == ZKMI_CURVE_BN128 ? group_scale_g1_run<Bn254Fq>(d_in, d_out, n, d) : group_scale_g1_run<Compact<Bls12381Fq>>(d_in, d_out, n, d);
}
static int group_scale_check(int curve, int group, const uint8_t* k_mont) {
    if ((curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) || (group != 1 && group != 2)) return fail(ZKMI_ERR_INVALID, "group scale: unknown curve or group");
    if (!k_mont) return fail(ZKMI_ERR_INVALID, "group scale: null argument");
    if (pipeline_busy()) return fail(ZKMI_ERR_INVALID, "group scale: a pipeline slot holds work in flight (collect it first)");
    return ZKMI_OK;
}

// ---- phase-2 host helpers -----------------------------------------------------------------------------------------------------------------------
static int hex_le_bytes(const char* hex, uint8_t* out, int cap) {          // big-endian hex digits -> little-endian bytes; returns the bit length
    const int nd = (int)strlen(hex);
    memset(out, 0, cap);
    for (int i = 0; i < nd; i++) {
        const char c = hex[nd - 1 - i];
        const int v = c <= '9' ? c - '0' : c - 'a' + 10;
        out[i / 2] |= (uint8_t)(v << (4 * (i & 1)));
    }
    int bits = 8 * cap;
    while (bits && !((out[(bits - 1) / 8] >> ((bits - 1) % 8)) & 1)) bits--;
    return bits;
}
// the cofactors of the reference's curve records (min.js: cofactorG1 / cofactorG2 of buildBn128 and buildBls12381); BN254 G1 has none
static const char* cofactor_hex(int curve, int group) {
    if (curve == ZKMI_CURVE_BN128) return group == 1 ? "" : "30644e72e131a029b85045b68181585e06ceecda572a2489345f2299c0f9fa8d";
    return group == 1 ? "396c8c005555e1568c00aaab0000aaab"
                      : "5d543a95414e7f1091d50792876a202cd91de4547085abaa68a205b2e5a7ddfa628f1cb4d9e82ef21537e293a6691ae1616ec6e786f0c70cf1c38e31c7238e5";
}
template <int L> struct Phase2Curve {
    host::HField<L> Fq;
    host::HField2<L> Fq2;
    host::HField<4> Fr;
    int curve;
    // curve constant b: 3 (BN254 G1), 3 / (9 + u) (BN254 G2), 4 (BLS12-381 G1), 4 (1 + u) (BLS12-381 G2)
    host::HFp<L> b1() const { return Fq.from_u64(curve == ZKMI_CURVE_BN128 ? 3 : 4); }
    host::HFp2<L> b2() const {
        if (curve == ZKMI_CURVE_BN128) return Fq2.mul(host::HFp2<L>{b1(), Fq.zero()}, Fq2.inv(host::HFp2<L>{Fq.from_u64(9), Fq.One()}));
        return host::HFp2<L>{b1(), b1()};
    }
};
template <class FqC, class FrC> static Phase2Curve<FqC::N / 2> phase2_curve(int curve) {
    Phase2Curve<FqC::N / 2> c;
    c.Fq = host::HField<FqC::N / 2>::template from_cfg<FqC>();
    c.Fq2.F = c.Fq;
    c.Fr = host::HField<4>::from_cfg<FrC>();
    c.curve = curve;
    return c;
}
template <class FT> static void put_affine(const FT& F, const typename host::HCurve<FT>::P& p, uint8_t* out) {
    host::HCurve<FT> cv{F};
    typename FT::E x, y;
    cv.to_affine(p, x, y);
    memcpy(out, &x, sizeof x); memcpy(out + sizeof x, &y, sizeof y);
}
template <class FT> static void point_mul_host(const FT& F, const host::HField<4>& Fr, const uint8_t* affine, const uint8_t* k_mont, uint8_t* out) {
    host::HCurve<FT> cv{F};
    typename FT::E x, y;
    memcpy(&x, affine, sizeof x); memcpy(&y, affine + sizeof x, sizeof y);
    host::HFp<4> k;
    memcpy(k.v, k_mont, 32);
    const host::HFp<4> kn = Fr.from_mont(k);
    put_affine(F, cv.mul_bits(cv.from_affine(x, y), (const uint8_t*)kn.v, 256), out);
}
template <class FqC, class FrC> static int key_from_seed(int curve, const uint32_t* seed, uint8_t* prv, uint8_t* g1_s, uint8_t* g1_sx) {
    const auto c = phase2_curve<FqC, FrC>(curve);
    phase2::ChaCha rng(seed);
    const host::HFp<4> k = phase2::field_from_rng(c.Fr, rng);
    uint8_t cof[64];
    const int bits = hex_le_bytes(cofactor_hex(curve, 1), cof, sizeof cof);
    uint8_t s[2 * FqC::N * 4];
    put_affine(c.Fq, phase2::point_from_rng(c.Fq, c.b1(), cof, bits, rng), s);
    memcpy(prv, k.v, 32);
    memcpy(g1_s, s, sizeof s);
    point_mul_host(c.Fq, c.Fr, s, prv, g1_sx);
    return ZKMI_OK;
}
// keypair.createPTauKey without its G2 halves: three Fr.fromRng (tau, alpha, beta), then per key G1.fromRng on the same generator and the product
template <class FqC, class FrC> static int ptau_key_from_seed(int curve, const uint32_t* seed, uint8_t* prv3, uint8_t* g1_s3, uint8_t* g1_sx3) {
    const auto c = phase2_curve<FqC, FrC>(curve);
    constexpr size_t sG1 = 2 * FqC::N * 4;
    phase2::ChaCha rng(seed);
    for (int i = 0; i < 3; i++) { const host::HFp<4> k = phase2::field_from_rng(c.Fr, rng); memcpy(prv3 + 32 * i, k.v, 32); }
    uint8_t cof[64];
    const int bits = hex_le_bytes(cofactor_hex(curve, 1), cof, sizeof cof);
    for (int i = 0; i < 3; i++) {
        put_affine(c.Fq, phase2::point_from_rng(c.Fq, c.b1(), cof, bits, rng), g1_s3 + sG1 * i);
        point_mul_host(c.Fq, c.Fr, g1_s3 + sG1 * i, prv3 + 32 * i, g1_sx3 + sG1 * i);
    }
    return ZKMI_OK;
}
template <class FqC, class FrC> static int hash_to_g2(int curve, const uint8_t* transcript, uint8_t* out) {
    const auto c = phase2_curve<FqC, FrC>(curve);
    uint32_t seed[8];
    for (int i = 0; i < 8; i++) seed[i] = ((uint32_t)transcript[4 * i] << 24) | ((uint32_t)transcript[4 * i + 1] << 16) | ((uint32_t)transcript[4 * i + 2] << 8) | transcript[4 * i + 3];
    phase2::ChaCha rng(seed);
    uint8_t cof[64];
    const int bits = hex_le_bytes(cofactor_hex(curve, 2), cof, sizeof cof);
    put_affine(c.Fq2, phase2::point_from_rng(c.Fq2, c.b2(), cof, bits, rng), out);
    return ZKMI_OK;
}
template <class FqC, class FrC> static int point_mul(int curve, int group, const uint8_t* affine, const uint8_t* k_mont, uint8_t* out) {
    const auto c = phase2_curve<FqC, FrC>(curve);
    if (group == 1) point_mul_host(c.Fq, c.Fr, affine, k_mont, out); else point_mul_host(c.Fq2, c.Fr, affine, k_mont, out);
    return ZKMI_OK;
}
static size_t pages_bytes(const zkmi_pages& pg) { size_t t = 0; for (int i = 0; i < pg.n_pages; i++) t += pg.len[i]; return t; }

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zkmi_group_scale_dev(int curve, int group, const void* d_in, void* d_out, size_t n, const uint8_t* k_mont) {
    ZK_TRY(require_ctx());
    ZK_TRY(group_scale_check(curve, group, k_mont));
    if (n && (!d_in || !d_out)) return fail(ZKMI_ERR_INVALID, "group scale: null buffer");
    return group_scale_dispatch(curve, group, d_in, d_out, n, k_mont);
}
int zkmi_group_scale(int curve, int group, zkmi_pages in, uint8_t* const* out_ptr, const size_t* out_len, int n_out_pages, size_t n, const uint8_t* k_mont) {
    ZK_TRY(require_ctx());
    ZK_TRY(group_scale_check(curve, group, k_mont));
    if (n >= (1ull << 31)) return fail(ZKMI_ERR_UNSUPPORTED, "group scale: at most 2^31 - 1 points");
    const size_t bytes = n * 2 * group * n8q_of(curve);
    if (pages_bytes(in) < bytes) return fail(ZKMI_ERR_INVALID, "input buffer shorter than n elements");
    if (!n) return ZKMI_OK;
    if (group == 2) return zkmi_group_batch_apply_key(curve, 2, in, out_ptr, out_len, n_out_pages, n, k_mont, (const uint8_t*)fr_one(curve).v);
    void* d_buf;
    ZK_TRY(ws_get("api.gscale", bytes, &d_buf));
    ZK_TRY(upload_pages(in, bytes, d_buf));
    ZK_TRY(group_scale_dispatch(curve, group, d_buf, d_buf, n, k_mont));
    return download_pages(d_buf, bytes, out_ptr, out_len, n_out_pages);
}
int zkmi_group_scale_recode(int curve, const uint8_t* k_mont, int8_t* digits, int* n_digits) {
    if ((curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) || !k_mont || !digits || !n_digits) return fail(ZKMI_ERR_INVALID, "group scale recode: bad argument");
    const ScaleDigits d = digits_of(curve, k_mont);
    for (uint32_t j = 0; j < d.n; j++) { const uint32_t t = scale_digit(d, j); digits[j] = (t & 1u) ? ((t & 2u) ? -1 : 1) : 0; }
    *n_digits = (int)d.n;
    return ZKMI_OK;
}

int zkmi_phase2_key_from_seed(int curve, const uint32_t* seed8, uint8_t* prv_key, uint8_t* g1_s, uint8_t* g1_sx) {
    if ((curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) || !seed8 || !prv_key || !g1_s || !g1_sx) return fail(ZKMI_ERR_INVALID, "phase2_key_from_seed: bad argument");
    return curve == ZKMI_CURVE_BN128 ? key_from_seed<Bn254Fq, Bn254Fr>(curve, seed8, prv_key, g1_s, g1_sx) : key_from_seed<Bls12381Fq, Bls12381Fr>(curve, seed8, prv_key, g1_s, g1_sx);
}
int zkmi_ptau_key_from_seed(int curve, const uint32_t* seed8, uint8_t* prv_keys, uint8_t* g1_s, uint8_t* g1_sx) {
    if ((curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) || !seed8 || !prv_keys || !g1_s || !g1_sx) return fail(ZKMI_ERR_INVALID, "ptau_key_from_seed: bad argument");
    return curve == ZKMI_CURVE_BN128 ? ptau_key_from_seed<Bn254Fq, Bn254Fr>(curve, seed8, prv_keys, g1_s, g1_sx) : ptau_key_from_seed<Bls12381Fq, Bls12381Fr>(curve, seed8, prv_keys, g1_s, g1_sx);
}
int zkmi_phase2_hash_to_g2(int curve, const uint8_t* transcript64, uint8_t* g2_sp) {
    if ((curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) || !transcript64 || !g2_sp) return fail(ZKMI_ERR_INVALID, "phase2_hash_to_g2: bad argument");
    return curve == ZKMI_CURVE_BN128 ? hash_to_g2<Bn254Fq, Bn254Fr>(curve, transcript64, g2_sp) : hash_to_g2<Bls12381Fq, Bls12381Fr>(curve, transcript64, g2_sp);
}
int zkmi_point_mul(int curve, int group, const uint8_t* affine, const uint8_t* k_mont, uint8_t* out_affine) {
    if ((curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) || (group != 1 && group != 2) || !affine || !k_mont || !out_affine) return fail(ZKMI_ERR_INVALID, "point_mul: bad argument");
    return curve == ZKMI_CURVE_BN128 ? point_mul<Bn254Fq, Bn254Fr>(curve, group, affine, k_mont, out_affine) : point_mul<Bls12381Fq, Bls12381Fr>(curve, group, affine, k_mont, out_affine);
}

}  // extern "C"
