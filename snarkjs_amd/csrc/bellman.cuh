// snarkjs_amd/csrc/bellman.cuh — the H basis change of a Bellman-format phase-2 round trip for gfx950: the two ends of the group FFT that
// zKey.exportBellman (src/zkey_export_bellman.js:43-52) and zKey.importBellman (src/zkey_import_bellman.js:133-142) run over section 9 of a Groth16 key.
//
//   export   out_i = (-2 w^i) FFT(in)_i            i < n - 1     w = Fr.w[log n + 1]; uncompressed big-endian points out
//   import   out   = iFFT([c_j P_j ..., infinity])   j < n - 1     c_j = -(2 n)^-1 w^-j: the 1 / n of the inverse sits in the one scalar of a point
// The butterflies between the ends are k_gfft_stage (gfft.cuh) on its work array of XYZZ points in the reference's R-form, unchanged. The ends:
//   k_bellman_scalars        first * inc^i in normal form, one lane per scalar, derived as k_g_apply_key derives it.
//   k_bellman_import_load    one lane per point: big-endian normal-form bytes -> R'-form limbs (one product with R'^2), c_j P_j in the all-odd signed binary form of
//                            mul_each_lane29 (ptau_contribute.cuh: no digit-dependent branch, so the different scalars of a wave do not diverge), stored in R-form
//                            at the bit-reversed place; the last slot and an all-zero input are the point at infinity.
//   k_bellman_export_twist   one lane per point, in place on the work array. The FFT leaves XYZZ points, mul_each_lane29 wants an affine base: (X, Y) IS an
//                            affine point of the isomorphic curve y^2 = x^3 + b ZZZ^2 ((x, y) -> (x ZZ, y ZZZ), a group isomorphism because ZZ^3 = ZZZ^2), and
//                            the a = 0 formulas of dbl_xyzz29 / madd29 never read b. So k (X, Y) runs on that curve and the result returns by one product each
//                            on ZZ and ZZZ: no inversion before the multiplication.
//   k_bellman_export_store   XYZZ (R'-form words) -> affine -> big-endian normal-form bytes, SCALE_INV points per lane behind ONE inversion (Montgomery's trick
//                            on ZZZ, the sweeps of scale_affine_group29). A point at infinity takes no part in its group's product and is written as zeros.
// A lane of a wave cannot share an inversion with its neighbours at a profit (the wave pays for the one lane that inverts as for all), hence the store is a
// launch of its own with a quarter of the lanes. The per-lane routines are __host__ __device__: tools/bellman_hosttest.hip runs them on the CPU.
#pragma once
#include "ptau_contribute.cuh"

namespace zkmi {

// R'^2 mod p (R' = 2^(B NL) of field29.cuh) as N canonical words, by value in the kernel arguments: a normal-form value times it is that value's R'-form
template <int N> struct BellmanRR { uint32_t w[N]; };

ZK_HD uint32_t bswap32_hd(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }

// N big-endian normal-form words at src -> R'-form limbs, below 1.1 p and normalised. A file from outside may hold a coordinate of p or more: any value below
// 2^(32 N) (5.3 p on BN254) is taken as its residue, and a -DZK29_BOUNDS build carries that bound, not the canonical one, into the product
template <class C> ZK_HD Fp29<C> from_be_normal29(const uint32_t* src, const Fp29<C>& rr) {
    constexpr int N = C::N;
    uint32_t w[N];
#pragma unroll
    for (int i = 0; i < N; i++) w[i] = bswap32_hd(src[N - 1 - i]);
    Fp29<C> t = unpack29<C>(w);
#if defined(ZK29_SHADOW)
    b29::set(t, ldexp(1.0, 32 * N) / b29::pval<C>(), b29::lowmax<C>(), -1.0);
#endif
    return mul29(t, rr);
}
// R'-form limbs (any lazy value store_r256 takes) -> N big-endian normal-form words: one product with the plain integer 1 divides by R'
template <class C> ZK_HD void store_be_normal29(uint32_t* dst, const Fp29<C>& a_in) {
    constexpr int N = C::N;
    Fp29<C> a = a_in, k = zero29<C>();
    norm29(a);
    k.l[0] = 1u;
    Fp29<C> t = mul29(a, k);
    canon29(t);
    uint32_t w[N];
    pack29<C>(w, t);
#pragma unroll
    for (int i = 0; i < N; i++) dst[i] = bswap32_hd(w[N - 1 - i]);
}

// import, one point: the uncompressed point at src (2 N words, all-zero = infinity) times the scalar at k (8 words, normal form), as XYZZ words in the
// reference's R-form at dst (4 N words, all-zero = infinity): what k_gfft_stage loads
template <class C> ZK_HD void bellman_import_point29(const uint32_t* src, const uint32_t* k, const BellmanRR<C::N>& rr, uint32_t* dst) {
    constexpr int N = C::N;
    uint32_t nz = 0;
#pragma unroll
    for (int i = 0; i < 2 * N; i++) nz |= src[i];
    XYZZ29<C> acc;
    bool inf = true;
    if (nz) {
        const Fp29<C> r2 = unpack29<C>(rr.w);
        Aff29<C> p;
        p.x = from_be_normal29<C>(src, r2); p.y = from_be_normal29<C>(src + N, r2);
        mul_each_lane29(acc, inf, p, k);
    }
    store_xyzz29<C, false>(dst, acc, inf);
}

ZK_HD uint32_t bitrev32_hd(uint32_t v, uint32_t bits) {                                 // 1 <= bits <= 32
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(v) >> (32 - bits);
#else
    uint32_t r = 0;
    for (uint32_t b = 0; b < bits; b++) r |= ((v >> b) & 1u) << (bits - 1 - b);
    return r;
#endif
}
// slot i of the import's load, n = 2^log_n (log_n >= 1): work[bitrev(i)] = scalars[i] * in_u[i] for i < n - 1, the point at infinity for i = n - 1, the
// coefficient export dropped (in_u holds n - 1 points)
template <class C> ZK_HD void bellman_import_slot29(const uint32_t* in_u, const uint32_t* scalars, const BellmanRR<C::N>& rr, uint32_t* work, uint32_t i, uint32_t n, uint32_t log_n) {
    constexpr int N = C::N;
    uint32_t* dst = work + (size_t)bitrev32_hd(i, log_n) * 4 * N;
    if (i == n - 1) {
#pragma unroll
        for (int k = 0; k < N; k++) reinterpret_cast<uint4*>(dst)[k] = make_uint4(0, 0, 0, 0);
        return;
    }
    bellman_import_point29<C>(in_u + (size_t)i * 2 * N, scalars + (size_t)i * 8, rr, dst);
}

// export, one point, in place: the XYZZ point at pt (4 N words in R-form as k_gfft_stage stores it, ZZ all-zero = infinity) times the scalar at k, left as
// XYZZ words in R'-form (all-zero = infinity): what bellman_affine_u_group29 reads
template <class C> ZK_HD void bellman_export_point29(uint32_t* pt, const uint32_t* k) {
    constexpr int N = C::N;
    XYZZ29<C> acc;
    bool inf = true;
    if (!xyzz29_words_inf<C>(pt)) {
        Aff29<C> p;
        p.x = from_r256<C>(pt); p.y = from_r256<C>(pt + N);                             // an affine point of the isomorphic curve
        mul_each_lane29(acc, inf, p, k);
        if (!inf) { acc.ZZ = mul29(acc.ZZ, from_r256<C>(pt + 2 * N)); acc.ZZZ = mul29(acc.ZZZ, from_r256<C>(pt + 3 * N)); }      // and back
    }
    store_xyzz29<C, true>(pt, acc, inf);
}

// one step of the backward sweep (scale_affine_one29 of group_scale.cuh with the other store): inv = 1 / (product of the ZZZ of points 0 .. k that are not at
// infinity), pre_k = that product without point k
template <class C> ZK_HD void bellman_affine_u_one29(const uint32_t* src, uint32_t* dst, Fp29<C>& inv, const Fp29<C>& pre_k) {
    constexpr int N = C::N;
    if (xyzz29_words_inf<C>(src)) {
#pragma unroll
        for (int i = 0; i < 2 * N; i++) dst[i] = 0u;
        return;
    }
    const Fp29<C> i3 = mul29(inv, pre_k);
    inv = mul29(inv, load29_packed<C>(src + 3 * N));
    const Fp29<C> i2 = sqr29(mul29(load29_packed<C>(src + 2 * N), i3));
    store_be_normal29<C>(dst, mul29(load29_packed<C>(src), i2));
    store_be_normal29<C>(dst + N, mul29(load29_packed<C>(src + N), i3));
}
// cnt <= SCALE_INV points as bellman_export_point29 left them (4 N words each) -> uncompressed big-endian points (2 N words each, all-zero = infinity)
template <class C> ZK_HD void bellman_affine_u_group29(const uint32_t* in, uint32_t* out, uint32_t cnt) {
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
    if (cnt > 3) bellman_affine_u_one29<C>(in + 12 * N, out + 6 * N, inv, pre3);
    if (cnt > 2) bellman_affine_u_one29<C>(in + 8 * N, out + 4 * N, inv, pre2);
    if (cnt > 1) bellman_affine_u_one29<C>(in + 4 * N, out + 2 * N, inv, pre1);
    bellman_affine_u_one29<C>(in, out, inv, pre0);
}

#if defined(__HIPCC__)
// scalars[i] = first * inc^i out of Montgomery form; `consts` = first | inc | inc^256 (Montgomery), the exponent split of k_g_apply_key (gfft.cuh)
template <class FrC> __global__ void __launch_bounds__(256)
k_bellman_scalars(uint32_t* __restrict__ scalars, uint32_t n, const uint32_t* __restrict__ consts) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Fp<FrC> first = fp_load<FrC>(consts), inc = fp_load<FrC>(consts + 8), inc256 = fp_load<FrC>(consts + 16);
    fp_store<FrC>(scalars + (size_t)i * 8, fp_from_mont(fp_mul(first, fp_mul(fp_pow_u32(inc256, i >> 8), fp_pow_u32(inc, i & 255u)))));
}
// one lane per slot of bellman_import_slot29
template <class C> __global__ void __launch_bounds__(256)
k_bellman_import_load(const uint32_t* __restrict__ in_u, const uint32_t* __restrict__ scalars, uint32_t* __restrict__ work, uint32_t n, uint32_t log_n, const BellmanRR<C::N> rr) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bellman_import_slot29<C>(in_u, scalars, rr, work, i, n, log_n);
}
// work[i] = scalars[i] * work[i] for i < m (R-form in, R'-form out)
template <class C> __global__ void __launch_bounds__(256)
k_bellman_export_twist(uint32_t* __restrict__ work, const uint32_t* __restrict__ scalars, uint32_t m) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    bellman_export_point29<C>(work + (size_t)i * 4 * C::N, scalars + (size_t)i * 8);
}
// out_u[i] = affine(work[i]) for i < m
template <class C> __global__ void __launch_bounds__(256)
k_bellman_export_store(const uint32_t* __restrict__ work, uint32_t* __restrict__ out_u, uint32_t m) {
    constexpr int N = C::N;
    const uint64_t i0 = (uint64_t)(blockIdx.x * 256 + threadIdx.x) * SCALE_INV;
    if (i0 >= m) return;
    const uint32_t left = m - (uint32_t)i0;
    bellman_affine_u_group29<C>(work + i0 * 4 * N, out_u + i0 * 2 * N, left < (uint32_t)SCALE_INV ? left : (uint32_t)SCALE_INV);
}
#endif

}  // namespace zkmi
