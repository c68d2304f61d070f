// snarkjs_amd/csrc/ptau_contribute.cuh — out_i = k_i * P_i for affine G1 points with a DIFFERENT scalar in every lane, for gfx950.
//
// The shape of phase 1 of a ceremony (src/powersoftau_contribute.js:135, src/powersoftau_beacon.js: every section through G.batchApplyKey(buff, first,
// inc), 5 * 2^power points with the scalar first * inc^i). The general kernel k_g_apply_key (gfft.cuh) recodes each lane's scalar as a non-adjacent form and
// branches on its digits, so at nearly every bit some lane of a wave adds while the others wait. Here every lane runs the SAME steps whatever its scalar:
// the all-odd signed binary form. For odd k < 2^255
//     k = sum_{j < 255} d_j 2^j,   d_254 = +1,   d_j = +1 if bit j + 1 of k is set, else -1   (j < 254)
// (2^254 + sum_{t = 1}^{254} b_t 2^t - (2^254 - 1) = k), so digit j is read straight from bit j + 1 of the scalar: no recoding pass, no digit array.
// An even k runs as k + 1 = k | 1, whose bits above bit 0 are those of k, and ends with one mixed addition of -P under the lane's predicate.
//   k_group_mul_each      one lane per point: acc = P, then 254 times acc = 2 acc (dbl_xyzz29), acc += +-P (madd29) on the limbs of field29.cuh. The prefix
//                         after digit j is the odd integer next to k / 2^j, below r for every k < r, so the accumulator leaves the generic branch of madd29
//                         only at the last digit of k + 1 = r (k = r - 1: the cancelling branch, then -P is added to infinity) and of k = 0 (acc = P, then
//                         the cancelling branch). madd29 is complete, so no scalar in [0, 2^255) needs a case of its own.
//   k_group_scale_affine  (group_scale.cuh, unchanged) XYZZ -> affine, SCALE_INV points behind one inversion.
// The per-lane routines are __host__ __device__: tools/ptau_contribute_hosttest.hip runs them on the CPU against the oracle.
#pragma once
#include "group_scale.cuh"

namespace zkmi {

// limb-wise choice between two elements; the worst-case bounds of a -DZK29_BOUNDS build cover both
template <class C> ZK_HD Fp29<C> sel29(bool take_a, const Fp29<C>& a, const Fp29<C>& b) {
    Fp29<C> r = b;
#pragma unroll
    for (int i = 0; i < Lim29<C>::NL; i++) r.l[i] = take_a ? a.l[i] : b.l[i];
#if defined(ZK29_SHADOW)
    b29::set(r, fmax(a.bv, b.bv), fmax(a.bl, b.bl), (a.bt < 0 || b.bt < 0) ? -1.0 : fmax(a.bt, b.bt));
#endif
    return r;
}

// acc = k p (p affine and not the point at infinity, coordinates as from_r256 leaves them); k = eight 32-bit words, least significant first, below 2^255
// (bit 255 is not read); inf = the result is the point at infinity
template <class C> ZK_HD void mul_each_lane29(XYZZ29<C>& acc, bool& inf, const Aff29<C>& p, const uint32_t* k) {
    acc.X = p.x; acc.Y = p.y; acc.ZZ = one29<C>(); acc.ZZZ = one29<C>();                // digit 254 = +1
    inf = false;
    Aff29<C> q;
    q.x = p.x;
    uint32_t w0 = 0;
#pragma unroll 1
    for (int w = 7; w >= 0; w--) {
        const uint32_t kw = k[w];                                                       // one word per 32 digits: never an indexed register array
        if (w == 0) w0 = kw;
        const int hi = w == 7 ? 30 : 31, lo = w == 0 ? 1 : 0;                           // bits 254 .. 1 = digits 253 .. 0
#pragma unroll 1
        for (int b = hi; b >= lo; b--) {
            // an accumulator at infinity (no scalar below r brings one here) holds stale but admissible words: doubling them is harmless, madd29 replaces them
            dbl_xyzz29(acc);
            q.y = sel29<C>(((kw >> b) & 1u) != 0, p.y, neg29<C, 2>(p.y));               // 2 p - y <= 2, normalised: what madd29 asks of its operand
            madd29(acc, inf, q);
        }
    }
    if (!(w0 & 1u)) {                                                                   // even k ran as k + 1
        q.y = neg29<C, 2>(p.y);
        madd29(acc, inf, q);
    }
}

// one point of the kernel: the affine point at src (2 N words, the reference's format, all-zero = infinity) times the scalar at k (8 words, normal form), as
// XYZZ words in R'-form at dst (4 N words, all-zero = infinity)
template <class C> ZK_HD void mul_each_point29(const uint32_t* src, const uint32_t* k, uint32_t* dst) {
    constexpr int N = C::N;
    uint32_t nz = 0;
#pragma unroll
    for (int i = 0; i < N / 2; i++) { const uint4 v = reinterpret_cast<const uint4*>(src)[i]; nz |= v.x | v.y | v.z | v.w; }
    XYZZ29<C> acc;
    bool inf = true;
    if (nz) {
        Aff29<C> p;
        p.x = from_r256<C>(src); p.y = from_r256<C>(src + N);
        mul_each_lane29(acc, inf, p, k);
    }
    store_xyzz29<C, true>(dst, acc, inf);
}

#if defined(__HIPCC__)
template <class C> __global__ void __launch_bounds__(256)
k_group_mul_each(const uint32_t* __restrict__ in, const uint32_t* __restrict__ scalars, uint32_t* __restrict__ work, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    mul_each_point29<C>(in + (size_t)i * 2 * C::N, scalars + (size_t)i * 8, work + (size_t)i * 4 * C::N);
}
#endif

}  // namespace zkmi
