// snarkjs_amd/csrc/plonk_verify.cuh — the per-proof PLONK check (src/plonk_verify.js:29-123 of snarkjs 0.7.6) for BN254 and BLS12-381, gfx950.
//
// One proof per lane, in the reference's order: the nine commitments decoded as G1.fromObject does and checked on the curve (-2), the
// public signals below r (-1), the six Fiat-Shamir challenges by Keccak-256 (src/Keccak256Transcript.js: points as x | y big-endian standard
// form, the point at infinity as zero bytes, scalars 32 bytes big-endian, challenge = digest mod r), xi^n, Z_H(xi), the Lagrange evaluations,
// PI(xi), r0 and the scalars of D, F and E exactly as oracle/plonk_verify_oracle.py::verifier_values states them, then
//     A1 = Wxi + u Wxiw,    B1 = xi Wxi + u xi w Wxiw + F - E,    e(-A1, X_2) e(B1, [1]_2) == 1.
// Both G2 arguments are fixed per key: a lane walks no G2 point, it reads two line tables (pairing.cuh g2_line_table / miller_multi).
//
// B1 is ONE interleaved double-and-add (Straus, shared doublings) over 18 bases — Qm Ql Qr Qo Qc S1 S2 S3, the G1 generator, A B C Z T1 T2
// T3 Wxi Wxiw — with the scalars collected per base first; only the group element matters, so D, F and E are never formed. Per lane that is
// 255 doublings and one mixed addition per set scalar bit (about 18 x 127); A1 is a 255-bit double-and-add of Wxiw by u plus one addition.
// Lanes of a wavefront disagree on which bits are set, so a wavefront pays nearly every addition slot.
//
// Lagrange evaluations: L_i = w^(i-1) Z_H(xi) / (n (xi - w^(i-1))), eight denominators per inversion (Montgomery's trick); the values are
// the oracle's. xi equal to a power of w would need a hash output that hits a root of unity; the reference divides by zero there too.
//
// The reference's "Proof evaluations are not valid" test reads the already reduced Montgomery bytes, so it cannot fire: evaluations are
// reduced modulo r here as Fr.fromObject reduces them, and code -4 stays reserved.
//
// Like pairing.cuh this is __device__ code that also compiles for the host (tools/plonk_verify_hosttest.hip, __device__ defined away).
#pragma once
#include "kzg_verify.cuh"

namespace zkmi {

// ---- per verifying key ----------------------------------------------------------------------------------------------------------------
enum { PLONKV_VALID = 1, PLONKV_INVALID = 0, PLONKV_BAD_PUBLIC = -1, PLONKV_BAD_POINT = -2 };      // -3: wrong signal count (whole call), -4 reserved
constexpr int PLONK_BASES = 18, PLONK_KEY_BASES = 9;

template <class C> struct PlonkVk {
    using S = Fp<typename PairingCfg<C>::Fr>;
    Fp<C> base[PLONK_KEY_BASES][2];            // Qm Ql Qr Qo Qc S1 S2 S3 and the G1 generator: affine, Montgomery, infinity all-zero
    uint32_t base_std[8][2 * C::N];            // x | y of the eight key points in standard form (the transcript's prefix)
    S omega, n_inv, k1, k2;                    // Fr.w[power], 1/n, k1, k2 (Montgomery)
    uint32_t power, n_public;
    uint32_t x2_inf;                           // X_2 is the point at infinity: its pair contributes 1
    uint32_t bad;                              // a key point is not on its curve: the load is refused
};
template <class C> struct PlonkVkView {
    const PlonkVk<C>* vk;
    const Line<C>* tab_x2;                     // miller_lines<C>() each
    const Line<C>* tab_g2;
};
// what zkmi_plonk_verify_trace_dev reports for one proof: beta gamma alpha xi v1 u L1(xi) PI(xi) r0 (standard form), affine A1 and B1
// (x | y, standard form, infinity all-zero)
template <class C> struct PlonkTrace {
    uint32_t fr[9][8];
    uint32_t a1[2 * C::N], b1[2 * C::N];
};

template <class C> ZK_PAIR_OP void plonk_vk_prepare(const uint32_t* g1_xyz, const uint32_t* x2_xyz, const uint32_t* k1, const uint32_t* k2, const uint32_t* omega_mont,
                                                    uint32_t power, uint32_t n_public, const PairingConsts<C>* K, PlonkVk<C>* vk, Line<C>* tab_x2, Line<C>* tab_g2) {
    using S = typename PlonkVk<C>::S;
    constexpr int N = C::N;
    uint32_t bad = 0;
    for (int j = 0; j < 8; j++) {
        Affine<Fp<C>> P;
        const bool inf = decode_point(g1_xyz + 3 * N * j, P);
        if (!inf && !on_curve(P, K)) bad = 1;
        vk->base[j][0] = P.x;
        vk->base[j][1] = P.y;
        const Fp<C> sx = fp_from_mont(P.x), sy = fp_from_mont(P.y);
        for (int i = 0; i < N; i++) { vk->base_std[j][i] = sx.l[i]; vk->base_std[j][N + i] = sy.l[i]; }
    }
    if (kzg_vk_prepare(x2_xyz, omega_mont, power, K, vk->base[8], tab_x2, tab_g2, vk->omega, vk->n_inv, vk->x2_inf)) bad = 1;
    S a, b;
    for (int i = 0; i < 8; i++) { a.l[i] = k1[i]; b.l[i] = k2[i]; }
    vk->k1 = fp_to_mont(a);
    vk->k2 = fp_to_mont(b);
    vk->power = power;
    vk->n_public = n_public;
    vk->bad = bad;
}

// ---- per proof ------------------------------------------------------------------------------------------------------------------------
// proof record: A B C Z T1 T2 T3 Wxi Wxiw as (x, y, z) (27 Fq) | eval_a eval_b eval_c eval_s1 eval_s2 eval_zw (8 words each), standard form;
// pubs: vk.n_public x 8 words. tr (may be null) receives the intermediate values of a proof that passes the input checks.
template <class C> constexpr int plonk_record_words() { return 27 * C::N + 48; }
// With AGG the check stops before the pairing and hands over its two G1 points instead (the aggregated check, kzg_aggregate.cuh); the code is then
// PLONKV_VALID for "the input checks passed" (KzgPair: kzg_verify.cuh). Without it (the default: the per-proof kernels) the function is what it was.
template <class C, bool AGG = false>
ZK_PAIR_OP int plonk_verify_one(const uint32_t* rec, const uint32_t* pubs, const PlonkVkView<C>& V, const PairingConsts<C>* K, PlonkTrace<C>* tr, KzgPair<C>* pair = nullptr) {
    using Fr = typename PairingCfg<C>::Fr;
    using S = Fp<Fr>;
    constexpr int N = C::N;
    const PlonkVk<C>& vk = *V.vk;
    const uint32_t np = vk.n_public;
    Affine<Fp<C>> pb[9];                       // A B C Z T1 T2 T3 Wxi Wxiw
    bool ok = true;
    for (int j = 0; j < 9; j++) {
        const bool inf = decode_point(rec + 3 * N * j, pb[j]);
        ok = ok && (inf || on_curve(pb[j], K));
    }
    if (!ok) return PLONKV_BAD_POINT;
    for (uint32_t j = 0; j < np; j++)
        if (!public_below_r<C>(pubs + 8 * j)) return PLONKV_BAD_PUBLIC;
    S ev[6];                                   // a b c s1 s2 zw
    for (int j = 0; j < 6; j++) {
        S t;
        for (int i = 0; i < 8; i++) t.l[i] = rec[27 * N + 8 * j + i];
        ev[j] = fp_to_mont(t);
    }
    // challenges (:207-271)
    Keccak256 k;
    keccak_init(k);
    for (int j = 0; j < 8; j++) { keccak_be(k, vk.base_std[j], N); keccak_be(k, vk.base_std[j] + N, N); }
    for (uint32_t j = 0; j < np; j++) keccak_be(k, pubs + 8 * j, 8);
    for (int j = 0; j < 3; j++) keccak_point(k, pb[j]);
    const S beta = keccak_challenge<Fr>(k);
    keccak_init(k); keccak_fr(k, beta);
    const S gamma = keccak_challenge<Fr>(k);
    keccak_init(k); keccak_fr(k, beta); keccak_fr(k, gamma); keccak_point(k, pb[3]);
    const S alpha = keccak_challenge<Fr>(k);
    keccak_init(k); keccak_fr(k, alpha);
    for (int j = 4; j < 7; j++) keccak_point(k, pb[j]);
    const S xi = keccak_challenge<Fr>(k);
    keccak_init(k); keccak_fr(k, xi);
    for (int j = 0; j < 6; j++) keccak_fr(k, ev[j]);
    const S v1 = keccak_challenge<Fr>(k);
    keccak_init(k); keccak_point(k, pb[7]); keccak_point(k, pb[8]);
    const S u = keccak_challenge<Fr>(k);
    // xi^n, Z_H(xi), L_i(xi), PI(xi) (:273-307)
    const S one = fp_one<Fr>();
    S xin = xi;
    for (uint32_t i = 0; i < vk.power; i++) xin = fp_sqr(xin);
    const S zh = fp_sub(xin, one);
    const S zhn = fp_mul(zh, vk.n_inv);
    S pi = fp_zero<Fr>(), L1 = fp_zero<Fr>(), w = one;
    const uint32_t m = np ? np : 1;
    for (uint32_t at = 0; at < m; at += 8) {
        const uint32_t cnt = m - at < 8 ? m - at : 8;
        S num[8], den[8], pre[8];
        for (uint32_t i = 0; i < cnt; i++) {
            num[i] = fp_mul(w, zhn);
            den[i] = fp_sub(xi, w);
            pre[i] = i ? fp_mul(pre[i - 1], den[i]) : den[i];
            w = fp_mul(w, vk.omega);
        }
        S inv = fp_inv(pre[cnt - 1]);
        for (uint32_t i = cnt; i-- > 0;) {
            const S L = fp_mul(num[i], i ? fp_mul(inv, pre[i - 1]) : inv);
            inv = fp_mul(inv, den[i]);
            if (at + i == 0) L1 = L;
            if (at + i < np) {
                S x;
                for (int q = 0; q < 8; q++) x.l[q] = pubs[8 * (at + i) + q];
                pi = fp_sub(pi, fp_mul(fp_to_mont(x), L));
            }
        }
    }
    // r0 (:309-331) and the scalars of D, F, E (:333-403)
    const S a = ev[0], b = ev[1], c = ev[2], s1 = ev[3], s2 = ev[4], zw = ev[5];
    const S as1 = fp_add(fp_add(a, fp_mul(beta, s1)), gamma), bs2 = fp_add(fp_add(b, fp_mul(beta, s2)), gamma);
    const S perm = fp_mul(as1, bs2);
    const S e3 = fp_mul(fp_mul(fp_mul(perm, fp_add(c, gamma)), zw), alpha);
    const S l1a2 = fp_mul(L1, fp_sqr(alpha));
    const S r0 = fp_sub(fp_sub(pi, l1a2), e3);
    const S bxi = fp_mul(beta, xi);
    const S d2a = fp_mul(fp_mul(fp_mul(fp_add(fp_add(a, bxi), gamma), fp_add(fp_add(b, fp_mul(bxi, vk.k1)), gamma)), fp_add(fp_add(c, fp_mul(bxi, vk.k2)), gamma)), alpha);
    const S d2 = fp_add(fp_add(d2a, l1a2), u);
    const S d3 = fp_mul(perm, fp_mul(fp_mul(alpha, beta), zw));
    const S v2 = fp_mul(v1, v1), v3 = fp_mul(v2, v1), v4 = fp_mul(v3, v1), v5 = fp_mul(v4, v1);
    S e = fp_add(fp_mul(v1, a), fp_mul(v2, b));
    e = fp_add(e, fp_add(fp_mul(v3, c), fp_mul(v4, s1)));
    e = fp_add(e, fp_add(fp_mul(v5, s2), fp_mul(u, zw)));
    e = fp_sub(e, r0);
    const S zhx = fp_mul(zh, xin);
    S sc[PLONK_BASES];                         // per base, standard form: key bases first (the order of PlonkVk::base), then the proof's
    sc[0] = fp_mul(a, b); sc[1] = a; sc[2] = b; sc[3] = c; sc[4] = one; sc[5] = v4; sc[6] = v5; sc[7] = fp_neg(d3); sc[8] = fp_neg(e);
    sc[9] = v1; sc[10] = v2; sc[11] = v3; sc[12] = d2; sc[13] = fp_neg(zh); sc[14] = fp_neg(zhx); sc[15] = fp_neg(fp_mul(zhx, xin));
    sc[16] = xi; sc[17] = fp_mul(fp_mul(u, xi), vk.omega);
    for (int j = 0; j < PLONK_BASES; j++) sc[j] = fp_from_mont(sc[j]);
    // B1: Straus over the 18 bases
    XYZZ<Fp<C>> acc;
    pt_set_inf(acc);
    for (int bit = 254; bit >= 0; bit--) {
        acc = pt_dbl(acc);
        for (int j = 0; j < PLONK_BASES; j++)
            if ((sc[j].l[bit >> 5] >> (bit & 31)) & 1)
                pt_madd(acc, j < PLONK_KEY_BASES ? Affine<Fp<C>>{vk.base[j][0], vk.base[j][1]} : pb[j - PLONK_KEY_BASES]);
    }
    // A1 = Wxi + u Wxiw
    const S us = fp_from_mont(u);
    XYZZ<Fp<C>> acc_a;
    pt_set_inf(acc_a);
    for (int bit = 254; bit >= 0; bit--) {
        acc_a = pt_dbl(acc_a);
        if ((us.l[bit >> 5] >> (bit & 31)) & 1) pt_madd(acc_a, pb[8]);
    }
    pt_madd(acc_a, pb[7]);
    Fp<C> ax, ay, bx, by;
    const bool a_fin = xyzz_to_affine(acc_a, ax, ay), b_fin = xyzz_to_affine(acc, bx, by);
    if (tr) {
        const S t[9] = {beta, gamma, alpha, xi, v1, u, L1, pi, r0};
        for (int j = 0; j < 9; j++) {
            const S s = fp_from_mont(t[j]);
            for (int i = 0; i < 8; i++) tr->fr[j][i] = s.l[i];
        }
        const Fp<C> p[4] = {fp_from_mont(ax), fp_from_mont(ay), fp_from_mont(bx), fp_from_mont(by)};
        for (int i = 0; i < N; i++) { tr->a1[i] = p[0].l[i]; tr->a1[N + i] = p[1].l[i]; tr->b1[i] = p[2].l[i]; tr->b1[N + i] = p[3].l[i]; }
    }
    if constexpr (AGG) {
        *pair = KzgPair<C>{ax, ay, bx, by, a_fin, b_fin};
        return PLONKV_VALID;
    } else {
        // e(-A1, X_2) e(B1, [1]_2) == 1 (:405-421); pairs are passed as (-px, py)
        const FixedPair<C> f0{V.tab_x2, fp_neg(ax), fp_neg(ay), a_fin && !vk.x2_inf};
        const FixedPair<C> f1{V.tab_g2, fp_neg(bx), by, b_fin};
        Affine<Fp2<C>> none;
        f_set_zero(none.x);
        f_set_zero(none.y);
        const Fp12<C> f = miller_multi(none, ax, ay, false, f0, f1, K);
        return f12_is_one(final_exp(f, K)) ? PLONKV_VALID : PLONKV_INVALID;
    }
}

}  // namespace zkmi
