// snarkjs_amd/csrc/group_scale.cuh — out_i = k * P_i for ONE scalar k and many affine G1 points, for gfx950.
//
// The shape of phase 2 of a Groth16 ceremony (src/zkey_contribute.js:90-92, src/zkey_beacon.js:113-115: sections L and H times 1 / delta through
// G1.batchApplyKey with inc = 1). The general kernel k_g_apply_key (gfft.cuh) recodes a different scalar in every lane; here the scalar is recoded ONCE
// on the host as a non-adjacent form, most significant digit first, and travels by value in the kernel arguments, so the digit loop branches on scalar
// registers: every lane of every wave doubles and adds in step.
//   k_group_scale         one lane per point: XYZZ accumulator on the unsaturated limbs of field29.cuh, doublings dbl_xyzz29 and mixed additions madd29
//                         of +-P (msm29.cuh). Both handle an accumulator at infinity, so a digit stream that passes through r P (or k = 0) is exact.
//   k_group_scale_affine  XYZZ -> affine Montgomery, SCALE_INV points per lane behind ONE inversion (Montgomery's trick on ZZZ, as k_setup_affine of
//                         groth16_setup.cuh, on the same limbs as the first kernel). A point at infinity takes no part in its group's product.
// The per-lane routines are __host__ __device__ like the formulas they call: tools/group_scale_hosttest.hip runs them on the CPU against the oracle.
#pragma once
#include "msm29.cuh"

namespace zkmi {

constexpr int SCALE_INV = 4;                 // points per inversion
constexpr int SCALE_MAX_DIGITS = 256;        // a non-adjacent form is at most one digit longer than its scalar, and r < 2^255 on both curves

// two bits per digit, most significant digit first: digit j in bits 2 (j & 15) of w[j >> 4]; bit 0 = non-zero, bit 1 = negative
struct ScaleDigits { uint32_t w[SCALE_MAX_DIGITS / 16]; uint32_t n; };
ZK_HD uint32_t scale_digit(const ScaleDigits& d, uint32_t j) { return (d.w[j >> 4] >> (2 * (j & 15))) & 3u; }

// non-adjacent form of k (four 64-bit words, k < 2^255)
inline ScaleDigits scale_recode(const uint64_t k_in[4]) {
    uint64_t k[4] = {k_in[0], k_in[1], k_in[2], k_in[3]};
    uint8_t lsb_first[SCALE_MAX_DIGITS + 1];
    uint32_t n = 0;
    while (k[0] | k[1] | k[2] | k[3]) {
        uint8_t d = 0;
        if (k[0] & 1u) {
            if ((k[0] & 3u) == 1u) { d = 1; k[0] -= 1; }                                              // digit +1
            else { d = 3; for (int i = 0; i < 4; i++) if (++k[i]) break; }                            // digit -1: k + 1 carries
        }
        lsb_first[n++] = d;
        for (int i = 0; i < 4; i++) k[i] = (k[i] >> 1) | (i < 3 ? k[i + 1] << 63 : 0);
    }
    ScaleDigits out;
    for (uint32_t& w : out.w) w = 0;
    out.n = n;
    for (uint32_t j = 0; j < n; j++) out.w[j >> 4] |= (uint32_t)lsb_first[n - 1 - j] << (2 * (j & 15));
    return out;
}

// acc = k p (p affine and not the point at infinity, coordinates as from_r256 leaves them); inf = the result is the point at infinity
template <class C> ZK_HD void scale_lane29(XYZZ29<C>& acc, bool& inf, const Aff29<C>& p, const ScaleDigits& d) {
    inf = true;
    for (uint32_t j = 0; j < d.n; j++) {
        if (!inf) dbl_xyzz29(acc);
        const uint32_t t = scale_digit(d, j);
        if (t & 1u) {
            Aff29<C> q = p;
            if (t & 2u) q.y = neg29<C, 2>(p.y);                                   // 2 p - y <= 2, normalised: what madd29 asks of its operand
            madd29(acc, inf, q);
        }
    }
}

// a^(p - 2): R'-form in and out, a normalised and below 2 p
template <class C> ZK_HD Fp29<C> inv29(const Fp29<C>& a) {
    constexpr int NL = Lim29<C>::NL, B = Lim29<C>::B;
    Fp29<C> r = one29<C>();
#pragma unroll 1
    for (int i = NL - 1; i >= 0; i--) {
        const uint32_t e = Lim29<C>::p(i) - (i == 0 ? 2u : 0u);                   // p is odd and its low limb exceeds 2
#pragma unroll 1
        for (int b = B - 1; b >= 0; b--) {
            r = sqr29(r);
            if ((e >> b) & 1u) r = mul29(r, a);
        }
    }
    return r;
}

// one step of the backward sweep: point k of the group, inv = 1 / (product of the ZZZ of points 0 .. k that are not at infinity), pre_k = that product without point k
template <class C> ZK_HD void scale_affine_one29(const uint32_t* src, uint32_t* dst, Fp29<C>& inv, const Fp29<C>& pre_k) {
    constexpr int N = C::N;
    if (xyzz29_words_inf<C>(src)) {
#pragma unroll
        for (int i = 0; i < N / 2; i++) reinterpret_cast<uint4*>(dst)[i] = make_uint4(0, 0, 0, 0);
        return;
    }
    const Fp29<C> i3 = mul29(inv, pre_k);
    inv = mul29(inv, load29_packed<C>(src + 3 * N));
    const Fp29<C> i2 = sqr29(mul29(load29_packed<C>(src + 2 * N), i3));
    store_r256<C>(dst, mul29(load29_packed<C>(src), i2));
    store_r256<C>(dst + N, mul29(load29_packed<C>(src + N), i3));
}
// cnt <= SCALE_INV points as store_xyzz29<C, true> wrote them (4 N words each, all-zero = infinity) -> affine points in the reference's format (2 N words
// each, all-zero = infinity): x = X / ZZ, y = Y / ZZZ with 1 / ZZ = (ZZ / ZZZ)^2
template <class C> ZK_HD void scale_affine_group29(const uint32_t* in, uint32_t* out, uint32_t cnt) {
    constexpr int N = C::N;
    static_assert(SCALE_INV == 4, "the sweeps below are written out for four points");
    const Fp29<C> pre0 = one29<C>();
    Fp29<C> pre1 = pre0, pre2, pre3, run;
    if (!xyzz29_words_inf<C>(in)) pre1 = mul29(pre0, load29_packed<C>(in + 3 * N));
    pre2 = pre1;
    if (cnt > 1 && !xyzz29_words_inf<C>(in + 4 * N)) pre2 = mul29(pre1, load29_packed<C>(in + 4 * N + 3 * N));
    pre3 = pre2;
    if (cnt > 2 && !xyzz29_words_inf<C>(in + 8 * N)) pre3 = mul29(pre2, load29_packed<C>(in + 8 * N + 3 * N));
    run = pre3;
    if (cnt > 3 && !xyzz29_words_inf<C>(in + 12 * N)) run = mul29(pre3, load29_packed<C>(in + 12 * N + 3 * N));
    Fp29<C> inv = inv29(run);
    if (cnt > 3) scale_affine_one29<C>(in + 12 * N, out + 6 * N, inv, pre3);
    if (cnt > 2) scale_affine_one29<C>(in + 8 * N, out + 4 * N, inv, pre2);
    if (cnt > 1) scale_affine_one29<C>(in + 4 * N, out + 2 * N, inv, pre1);
    scale_affine_one29<C>(in, out, inv, pre0);
}

// one point of the first kernel: the affine point at src (2 N words, the reference's format, all-zero = infinity) times the digits, as XYZZ words in
// R'-form at dst (4 N words, all-zero = infinity)
template <class C> ZK_HD void scale_point29(const uint32_t* src, uint32_t* dst, const ScaleDigits& d) {
    constexpr int N = C::N;
    uint32_t nz = 0;
#pragma unroll
    for (int k = 0; k < N / 2; k++) { const uint4 v = reinterpret_cast<const uint4*>(src)[k]; nz |= v.x | v.y | v.z | v.w; }
    XYZZ29<C> acc;
    bool inf = true;
    if (nz) {
        Aff29<C> p;
        p.x = from_r256<C>(src); p.y = from_r256<C>(src + N);
        scale_lane29(acc, inf, p, d);
    }
    store_xyzz29<C, true>(dst, acc, inf);
}

#if defined(__HIPCC__)
template <class C> __global__ void __launch_bounds__(256)
k_group_scale(const uint32_t* __restrict__ in, uint32_t* __restrict__ work, uint32_t n, const ScaleDigits d) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    scale_point29<C>(in + (size_t)i * 2 * C::N, work + (size_t)i * 4 * C::N, d);
}

template <class C> __global__ void __launch_bounds__(256)
k_group_scale_affine(const uint32_t* __restrict__ work, uint32_t* __restrict__ out, uint32_t n) {
    constexpr int N = C::N;
    const uint64_t i0 = (uint64_t)(blockIdx.x * 256 + threadIdx.x) * SCALE_INV;
    if (i0 >= n) return;
    const uint32_t left = n - (uint32_t)i0;
    scale_affine_group29<C>(work + i0 * 4 * N, out + i0 * 2 * N, left < (uint32_t)SCALE_INV ? left : (uint32_t)SCALE_INV);
}
#endif

}  // namespace zkmi
