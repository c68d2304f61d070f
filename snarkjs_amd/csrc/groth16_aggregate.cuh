// snarkjs_amd/csrc/groth16_aggregate.cuh — the aggregated ("are all of these valid?") check of a Groth16 batch, gfx950.
//
// A proof is valid when e(-A, B) e(vk_x, gamma) e(C, delta) e(alpha, beta) == 1. Only gamma, delta and (alpha, beta) are fixed per key: B differs
// per proof. For a batch under one key and a 32-byte seed, with r_i the challenge of kzg_aggregate.cuh (agg_challenge) and E the lanes whose input
// checks pass (groth16_verify_one<C, true>, pairing.cuh):
//     F   = prod_E Miller(-r_i A_i, B_i)                one walked Miller loop per lane, r_i on the G1 side          (g16_agg_lane_one)
//     S_X = sum_E r_i vk_x_i,  S_C = sum_E r_i C_i,  s = sum_E r_i (192 bits)                                       (agg_scale, agg_block_sum)
//     ok  = every lane's code is 1  and  final_exp_chain(F Miller(S_X, gamma) Miller(S_C, delta) M(alpha, beta)^s) == 1   (g16_agg_tail)
// One final exponentiation and one pass over the gamma and delta tables per batch instead of one per proof; no final exponentiation in a lane.
//
// A lane whose input checks fail reports its code and contributes 1, infinity, infinity, 0. A pair with a point at infinity contributes 1 as in
// the per-proof kernel. On BLS12-381 the tail multiplies both sums by the G1 cofactor h (agg_clear_cofactor) and, so that the four factors stay
// one product of pairings, raises F M^s to h as well: the value tested is the batch's product to the power h, and gcd(h, r) = 1. The sums
// reported to a trace are the sums before that multiplication.
//
// Like kzg_aggregate.cuh this is __device__ code that also compiles for the host (tools/groth16_aggregate_hosttest.hip, __device__ defined away).
#pragma once
#include "kzg_aggregate.cuh"

namespace zkmi {

// What a lane, a block and a level of the reduction leave: the Fq12 product, the two sums (p = S_X, q = S_C), the sum of the challenges.
template <class C> struct G16Part {
    Fp12<C> f;
    AggPair<C> s;
    uint64_t r[3];
};
template <class C> ZK_DEV void g16_part_identity(G16Part<C>& o) {
    o.f = f12_one<C>();
    pt_set_inf(o.s.p);
    pt_set_inf(o.s.q);
    o.r[0] = o.r[1] = o.r[2] = 0;
}
ZK_DEV void g16_add3(uint64_t* a, const uint64_t* b) {
    unsigned __int128 c = 0;
    for (int k = 0; k < 3; k++) {
        c += (unsigned __int128)a[k] + b[k];
        a[k] = (uint64_t)c;
        c >>= 64;
    }
}

// One lane: the front half of the per-proof check, then r_i times A, C and vk_x and the walked Miller loop of (-r_i A, B). Returns the lane's
// code; o is the identity unless the code is AGG_ENTERED.
template <class C> ZK_DEV int g16_agg_lane_one(const uint32_t* rec, const uint32_t* pubs, uint32_t n_signals, const VkView<C>& vk, const PairingConsts<C>* K,
                                               const uint64_t* seed4, uint64_t i, G16Part<C>& o) {
    g16_part_identity(o);
    G16Front<C> fr;
    const int code = groth16_verify_one<C, true>(rec, pubs, n_signals, vk, K, &fr);
    if (code != AGG_ENTERED) return code;
    uint64_t lo, hi;
    agg_challenge(seed4, i, lo, hi);
    o.r[0] = lo;
    o.r[1] = hi;
    o.s.p = agg_scale<C>(fr.vx, fr.vy, !fr.x_inf, lo, hi);
    o.s.q = agg_scale<C>(fr.Cp.x, fr.Cp.y, !fr.c_inf, lo, hi);
    Fp<C> ax, ay;
    const bool a_fin = xyzz_to_affine(agg_scale<C>(fr.A.x, fr.A.y, !fr.a_inf, lo, hi), ax, ay);
    // the variable pair's P = -r_i A_i is passed as (-px, py), as groth16_verify_one passes -A; both fixed pairs are off
    const FixedPair<C> none{nullptr, ax, ay, false};
    o.f = miller_multi(fr.B, fp_neg(ax), fp_neg(ay), a_fin && !fr.b_inf, none, none, K);
    return code;
}

// Product of the T Fq12 values of a block (T a power of two, one per thread) by a tree in sh (T entries): the result is in sh[0] after the
// call. Every thread of the block must call it. On the host (T = 1) it is the identity.
template <class C, int T> ZK_DEV void g16_block_prod(Fp12<C>* sh, unsigned t, const Fp12<C>& mine) {
    sh[t] = mine;
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
    for (unsigned s = T / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] = f12_mul(sh[t], sh[t + s]);
        __syncthreads();
    }
#endif
}
// the same for the three-word sums of the challenges (sh: 3 T words)
template <int T> ZK_DEV void g16_block_add3(uint64_t* sh, unsigned t, const uint64_t* mine) {
    for (int k = 0; k < 3; k++) sh[3 * t + k] = mine[k];
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
    for (unsigned s = T / 2; s > 0; s >>= 1) {
        if (t < s) g16_add3(sh + 3 * t, sh + 3 * (t + s));
        __syncthreads();
    }
#endif
}

// a^e for a 192-bit e by plain square-and-multiply (a is an unreduced Miller value: not cyclotomic); e = 0 gives one
template <class C> ZK_PAIR_OP Fp12<C> f12_pow3(const Fp12<C>& a, const uint64_t* e) {
    Fp12<C> r = f12_one<C>();
    bool top = false;
    for (int i = 191; i >= 0; i--) {
        const bool bit = (e[i >> 6] >> (i & 63)) & 1;
        if (top) r = f12_sqr(r);
        if (bit) r = top ? f12_mul(r, a) : a;
        top = top || bit;
    }
    return r;
}

// what the tail reports: the verdict of the pairing check, the two sums (affine, standard form, x | y each, infinity all-zero, before the
// cofactor), s, and for a trace final_exp(F) (the plain one) in the oracle's w-basis, standard form
template <class C> struct G16AggResult {
    uint32_t pair_ok;
    uint32_t sx[2 * C::N], sc[2 * C::N];
    uint64_t s[3];
    uint32_t gt[12 * C::N];
};

// The tail, one lane: the batch's record -> the report. gt is filled only with `trace`.
template <class C> ZK_PAIR_OP void g16_agg_tail(const G16Part<C>& S, const VkView<C>& vk, const PairingConsts<C>* K, bool trace, G16AggResult<C>* out) {
    constexpr int N = C::N;
    Fp<C> x, y;
    (void)xyzz_to_affine(S.s.p, x, y);
    Fp<C> sx = fp_from_mont(x), sy = fp_from_mont(y);
    for (int i = 0; i < N; i++) { out->sx[i] = sx.l[i]; out->sx[N + i] = sy.l[i]; }
    (void)xyzz_to_affine(S.s.q, x, y);
    sx = fp_from_mont(x); sy = fp_from_mont(y);
    for (int i = 0; i < N; i++) { out->sc[i] = sx.l[i]; out->sc[N + i] = sy.l[i]; }
    for (int k = 0; k < 3; k++) out->s[k] = S.r[k];
    if (trace) {
        Fp<C> w[12];
        f12_to_wbasis(final_exp(S.f, K), w);
        for (int k = 0; k < 12; k++)
            for (int i = 0; i < N; i++) out->gt[k * N + i] = w[k].l[i];
    }
    Fp<C> px, py, qx, qy;
    const bool p_fin = xyzz_to_affine(agg_clear_cofactor<C>(S.s.p), px, py);
    const bool q_fin = xyzz_to_affine(agg_clear_cofactor<C>(S.s.q), qx, qy);
    // Miller(S_X, gamma) Miller(S_C, delta); pairs are passed as (-px, py)
    const FixedPair<C> g{vk.tab_gamma, fp_neg(px), py, p_fin && !vk.gamma_inf};
    const FixedPair<C> d{vk.tab_delta, fp_neg(qx), qy, q_fin && !vk.delta_inf};
    Affine<Fp2<C>> none;
    f_set_zero(none.x);
    f_set_zero(none.y);
    const Fp12<C> m = miller_multi(none, px, py, false, g, d, K);
    // F M(alpha, beta)^s, to the cofactor where the sums were multiplied by it
    Fp12<C> w = f12_mul(S.f, f12_pow3(*vk.mab, S.r));
    constexpr unsigned __int128 H = g1_cofactor<C>();
    if constexpr (H != 1) {
        const uint64_t h[3] = {(uint64_t)H, (uint64_t)(H >> 64), 0};
        w = f12_pow3(w, h);
    }
    out->pair_ok = f12_is_one(final_exp_chain(f12_mul(m, w), K)) ? 1u : 0u;
}

}  // namespace zkmi
