// snarkjs_amd/csrc/ptau_challenge.cuh — out_i = k_i * P_i for affine G2 points with a DIFFERENT scalar in every lane, for gfx950.
//
// The G2 section of a challenge response (src/powersoftau_challenge_contribute.js through applyKeyToChallengeSection of src/mpc_applykey.js: G2.batchApplyKey(buff,
// first, inc) between batchUtoLEM and batchLEMtoC). The twin of k_group_mul_each (ptau_contribute.cuh) over Fq2 = Fq[u] / (u^2 + 1), on the formulas the G2 MSM
// already runs (msm29.cuh):
//   k_group2_mul_each      one lane per point, the same all-odd signed binary form: acc = P, then 254 times acc = 2 acc (dbl29_lds), acc += +-P (madd29_lds), digit
//                          j read from bit j + 1 of the scalar, an even k run as k | 1 and mended by one addition of -P. The XYZZ accumulator is PARKED IN LDS
//                          (LdsAcc29, the layout and the lane counts of the bucket reduction, Reduce29G2): eight Fq values a lane do not fit the register file
//                          beside the operands of a product, and P itself stays in registers for the whole loop. A challenge file comes from outside, so P need
//                          not lie in the r-torsion: the prefix (the odd integer next to k / 2^j) times P may then be infinity or +-P in the middle of the loop.
//                          madd29_lds has both branches (acc = q: the doubling formulas, acc = -q: infinity) and an accumulator at infinity keeps admissible
//                          stale words that dbl29_lds may double and the next addition replaces. Neither twist has a point of order two (both cofactors are
//                          odd), so a doubling never leaves ZZ = 0 beside a clear flag.
//   k_group2_scale_affine  XYZZ over Fq2 -> affine LEM, SCALE_INV points behind ONE inversion in Fq2 (Montgomery's trick on ZZZ), the inverse as
//                          conj(a) / (a0^2 + a1^2) with one inv29. A point at infinity takes no part in its group's product.
// The per-lane routines are __host__ __device__: tools/ptau_challenge_hosttest.hip runs them on the CPU against the oracle.
#pragma once
#include "ptau_contribute.cuh"

namespace zkmi {

// lanes per block and LDS bytes per lane: the figures of the Fq2 bucket reduction, whose four-coordinate accumulator this is
template <class C> struct MulEachG2 {
    static constexpr int T = Reduce29G2<C>::T;
    typedef typename Reduce29G2<C>::Acc Acc;
    static constexpr size_t lds_bytes = Reduce29G2<C>::lds_bytes;
};

// acc (parked in A) = k p for p = (px, py) affine, not the point at infinity, coordinates as from_r256 leaves them; k as in mul_each_lane29
template <class C, class Acc> ZK_HD void mul_each_lane29_g2(const Acc& A, bool& inf, const F2x<C>& px, const F2x<C>& py, const uint32_t* k) {
    F2x<C> t;
    t.c0 = one29<C>(); t.c1 = zero29<C>();
    A.put(0, px); A.put(1, py); A.put(2, t); A.put(3, t);                               // digit 254 = +1
    inf = false;
    // ONE loop and one site of each formula (the code of a second madd29_lds is a quarter of the loop): step j = 254 .. 1 doubles and adds +-P by bit j
    // (digit j - 1); step 0 mends an even k, which ran as k | 1, by adding -P without a doubling, and an odd k leaves before it. The branches on j are scalar.
    uint32_t kw = k[7];
#pragma unroll 1
    for (int j = 254; j >= 0; j--) {
        if ((j & 31) == 31) kw = k[j >> 5];                                             // one word per 32 digits: never an indexed register array
        const bool plus = ((kw >> (j & 31)) & 1u) != 0;
        if (j == 0) { if (plus) break; }                                                // bit 0 clear: plus = false below, the addition of -P
        else dbl29_lds<C>(A);                                                           // at infinity: stale but admissible words, replaced by the addition
        ZK_SFENCE();
        t.c0 = sel29<C>(plus, py.c0, neg29<C, 2>(py.c0));                               // 2 p - y <= 2, normalised, per component
        t.c1 = sel29<C>(plus, py.c1, neg29<C, 2>(py.c1));
        ZK_SFENCE();
        madd29_lds<C>(A, inf, px, t);
        ZK_SFENCE();
    }
}

// one point of the kernel: the affine point at src (4 N words, the reference's format, all-zero = infinity) times the scalar at k (8 words, normal form), as
// XYZZ words in R'-form at dst (8 N words, all-zero = infinity)
template <class C, class Acc> ZK_HD void mul_each_point29_g2(const Acc& A, const uint32_t* src, const uint32_t* k, uint32_t* dst) {
    constexpr int N = C::N;
    uint32_t nz = 0;
#pragma unroll
    for (int i = 0; i < N; i++) { const uint4 v = reinterpret_cast<const uint4*>(src)[i]; nz |= v.x | v.y | v.z | v.w; }
    bool inf = true;
    if (nz) {
        F2x<C> px, py;
        px.c0 = from_r256<C>(src); px.c1 = from_r256<C>(src + N); py.c0 = from_r256<C>(src + 2 * N); py.c1 = from_r256<C>(src + 3 * N);
        mul_each_lane29_g2<C>(A, inf, px, py, k);
    }
    store_xyzz29_lds<C, Acc, true>(dst, A, inf);
}

// ---- XYZZ over Fq2 -> affine ---------------------------------------------------------------------------------------------------------------------------
template <class C> ZK_HD F2x<C> f2load_packed(const uint32_t* p) { return F2x<C>{load29_packed<C>(p), load29_packed<C>(p + C::N)}; }
// a b for b.c1 <= K (normalised operands)
template <class C, int K = 2> ZK_HD F2x<C> f2mul_k(const F2x<C>& a, const F2x<C>& b) { return f2mul(a, b, neg29<C, K>(b.c1)); }
// 1 / a = conj(a) / (a0^2 + a1^2) (u^2 = -1): components normalised and <= 2; the norm is one double product, so inv29 gets a value below 2 p
template <class C> ZK_HD F2x<C> f2inv(const F2x<C>& a) {
    const Fp29<C> ni = inv29(mul29_2(a.c0, a.c0, a.c1, a.c1));
    return F2x<C>{mul29(a.c0, ni), mul29(neg29<C, 2>(a.c1), ni)};
}
// one step of the backward sweep (scale_affine_one29 over Fq2): inv = 1 / (product of the ZZZ of points 0 .. k that are not at infinity), pre_k = that
// product without point k
template <class C> ZK_HD void scale_affine_one29_g2(const uint32_t* src, uint32_t* dst, F2x<C>& inv, const F2x<C>& pre_k) {
    constexpr int N = C::N;
    if (xyzz29_words_inf_g2<C>(src)) {
#pragma unroll
        for (int i = 0; i < N; i++) reinterpret_cast<uint4*>(dst)[i] = make_uint4(0, 0, 0, 0);
        return;
    }
    const F2x<C> i3 = f2mul_k<C>(inv, pre_k);
    inv = f2mul_k<C>(inv, f2load_packed<C>(src + 6 * N));
    const F2x<C> i2 = f2sqr<C, 2>(f2mul_k<C>(f2load_packed<C>(src + 4 * N), i3));       // c1 is a doubled product: <= 2.2
    const F2x<C> x = f2mul_k<C, 3>(f2load_packed<C>(src), i2), y = f2mul_k<C>(f2load_packed<C>(src + 2 * N), i3);
    store_r256<C>(dst, x.c0); store_r256<C>(dst + N, x.c1); store_r256<C>(dst + 2 * N, y.c0); store_r256<C>(dst + 3 * N, y.c1);
}
// cnt <= SCALE_INV points as store_xyzz29_lds<C, Acc, true> wrote them (8 N words each, all-zero = infinity) -> affine points in the reference's format
// (4 N words each, all-zero = infinity): x = X / ZZ, y = Y / ZZZ with 1 / ZZ = (ZZ / ZZZ)^2
template <class C> ZK_HD void scale_affine_group29_g2(const uint32_t* in, uint32_t* out, uint32_t cnt) {
    constexpr int N = C::N;
    static_assert(SCALE_INV == 4, "the sweeps below are written out for four points");
    F2x<C> pre0;
    pre0.c0 = one29<C>(); pre0.c1 = zero29<C>();
    F2x<C> pre1 = pre0, pre2, pre3, run;
    if (!xyzz29_words_inf_g2<C>(in)) pre1 = f2load_packed<C>(in + 6 * N);
    pre2 = pre1;
    if (cnt > 1 && !xyzz29_words_inf_g2<C>(in + 8 * N)) pre2 = f2mul_k<C>(pre1, f2load_packed<C>(in + 8 * N + 6 * N));
    pre3 = pre2;
    if (cnt > 2 && !xyzz29_words_inf_g2<C>(in + 16 * N)) pre3 = f2mul_k<C>(pre2, f2load_packed<C>(in + 16 * N + 6 * N));
    run = pre3;
    if (cnt > 3 && !xyzz29_words_inf_g2<C>(in + 24 * N)) run = f2mul_k<C>(pre3, f2load_packed<C>(in + 24 * N + 6 * N));
    F2x<C> inv = f2inv<C>(run);
    if (cnt > 3) scale_affine_one29_g2<C>(in + 24 * N, out + 12 * N, inv, pre3);
    if (cnt > 2) scale_affine_one29_g2<C>(in + 16 * N, out + 8 * N, inv, pre2);
    if (cnt > 1) scale_affine_one29_g2<C>(in + 8 * N, out + 4 * N, inv, pre1);
    scale_affine_one29_g2<C>(in, out, inv, pre0);
}

#if defined(__HIPCC__)
template <class C> __global__ void __launch_bounds__(MulEachG2<C>::T, 2)
k_group2_mul_each(const uint32_t* __restrict__ in, const uint32_t* __restrict__ scalars, uint32_t* __restrict__ work, uint32_t n) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_mul_each_g2[];
    const uint32_t i = blockIdx.x * MulEachG2<C>::T + threadIdx.x;
    if (i >= n) return;                                                                 // no barrier below: a lane owns its LDS words
    const typename MulEachG2<C>::Acc A{lds_mul_each_g2 + threadIdx.x};
    mul_each_point29_g2<C>(A, in + (size_t)i * 4 * C::N, scalars + (size_t)i * 8, work + (size_t)i * 8 * C::N);
}

template <class C> __global__ void __launch_bounds__(256)
k_group2_scale_affine(const uint32_t* __restrict__ work, uint32_t* __restrict__ out, uint32_t n) {
    constexpr int N = C::N;
    const uint64_t i0 = (uint64_t)(blockIdx.x * 256 + threadIdx.x) * SCALE_INV;
    if (i0 >= n) return;
    const uint32_t left = n - (uint32_t)i0;
    scale_affine_group29_g2<C>(work + i0 * 8 * N, out + i0 * 4 * N, left < (uint32_t)SCALE_INV ? left : (uint32_t)SCALE_INV);
}
#endif

}  // namespace zkmi
