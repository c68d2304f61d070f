// snarkjs_amd/csrc/fflonk_verify.cuh — the per-proof FFLONK check (src/fflonk_verify.js:28-137 of snarkjs 0.7.6) for BN254, gfx950.
//
// One proof per lane. The number of public signals is a property of the call and is tested by the caller first, as the reference tests it first
// (-3); a lane then tests, in the reference's order: C1 C2 W1 W2 decoded as G1.fromObject does and, with the key's C0, checked on the curve (-2),
// the public signals below r (-1), and the pairing (0 / 1). Values exactly as oracle/fflonk_verify_oracle.py::verifier_values states them:
// the five challenges beta gamma xiSeed alpha y by Keccak-256 (kzg_verify.cuh's sponge; the transcript's encoding is PLONK's), the roots
// S0 = h0 w8^i, S1 = h1 w4^i, S2 = h2 w3^i, S2' = h2 wr w3^i with h0 = xiSeed^3, h1 = xiSeed^6, h2 = xiSeed^8, xi = xiSeed^24, then Z_H, L_i, PI,
// r0 r1 r2, mulH0 mulH1 mulH2, the quotients q1 = alpha mulH0 / mulH1, q2 = alpha^2 mulH0 / mulH2, e = r0 + q1 r1 + q2 r2 and
//     A1 = C0 + q1 C1 + q2 C2 - e G - mulH0 W1 + y W2,        e(-A1, [1]_2) e(W2, X_2) == 1.
// Both G2 arguments are fixed per key: a lane reads two line tables (pairing.cuh g2_line_table / miller_multi).
//
// Inversions: the reference divides 22 + nPublic times. Here Z_H, the 8 + 4 + 6 Lagrange denominators of r0 r1 r2, mulH1, mulH2 and the first
// eight L_i denominators are ONE batch (Montgomery's trick, fflonk_batch_inv): one fp_inv over Fr for nPublic <= 8, one more per further eight
// public signals. A1 goes to affine with one fp_inv over Fq. final_exp has its own single inversion.
//
// A1 is ONE interleaved double-and-add (Straus, shared doublings) over five bases — C1 C2 G W1 W2 — plus one addition of C0; F, E and J are
// never formed. The five bases and scalars are named values, not arrays: the next bit of a scalar is its top bit, and the scalar is shifted
// left by one each step, so nothing is indexed by a loop variable and neither bases nor scalars need scratch memory for that reason.
//
// The reference's "Proof evaluations are not valid." test reads already reduced values, so it cannot fire: evaluations are reduced modulo r
// here as Fr.fromObject reduces them, and code -4 stays reserved. evaluations.inv is not part of a record: the verifier does not read it.
// y equal to a root, or xi equal to a power of w, would need a hash output that hits them; the reference divides by zero there too.
//
// Like plonk_verify.cuh this is __device__ code that also compiles for the host (tools/fflonk_verify_hosttest.hip, __device__ defined away).
#pragma once
#include "kzg_verify.cuh"

namespace zkmi {

enum { FFLONKV_VALID = 1, FFLONKV_INVALID = 0, FFLONKV_BAD_PUBLIC = -1, FFLONKV_BAD_POINT = -2 };      // -3: wrong signal count (whole call), -4 reserved
constexpr int FFLONK_EVALS = 15;               // ql qr qm qo qc s1 s2 s3 a b c z zw t1w t2w
constexpr int FFLONK_FIXED_DENS = 21;          // Z_H | 8 + 4 + 6 Lagrange denominators | mulH1 mulH2; up to eight L_i denominators follow

// ---- per verifying key ----------------------------------------------------------------------------------------------------------------
template <class C> struct FflonkVk {
    using S = Fp<typename PairingCfg<C>::Fr>;
    Fp<C> c0[2], g[2];                         // C0 and the G1 generator: affine, Montgomery, infinity all-zero
    uint32_t c0_std[2 * C::N];                 // x | y of C0 in standard form (the transcript's first item)
    S k1, k2, wr, omega, n_inv;                // Montgomery; omega = Fr.w[power]
    S w8p[8], w4p[4], w3p[3];                  // w8^0..7, w4^0..3, w3^0..2
    uint32_t power, n_public;
    uint32_t x2_inf;                           // X_2 is the point at infinity: its pair contributes 1
    uint32_t c0_bad;                           // C0 is not on the curve: the key loads and every proof under it gets -2, as the reference has it
    uint32_t bad;                              // X_2 is not on its curve: the load is refused
};
template <class C> struct FflonkVkView {
    const FflonkVk<C>* vk;
    const Line<C>* tab_x2;                     // miller_lines<C>() each
    const Line<C>* tab_g2;
};
// what zkmi_fflonk_verify_trace_dev reports for one proof: beta gamma xi alpha y r0 r1 r2 (standard form), affine A1 and B1 = W2
// (x | y, standard form, infinity all-zero)
template <class C> struct FflonkTrace {
    uint32_t fr[8][8];
    uint32_t a1[2 * C::N], b1[2 * C::N];
};

// consts: k1 k2 w3 w4 w8 wr, 8 words each, standard form
template <class C> ZK_PAIR_OP void fflonk_vk_prepare(const uint32_t* c0_xyz, const uint32_t* x2_xyz, const uint32_t* consts, const uint32_t* omega_mont, uint32_t power,
                                                     uint32_t n_public, const PairingConsts<C>* K, FflonkVk<C>* vk, Line<C>* tab_x2, Line<C>* tab_g2) {
    using Fr = typename PairingCfg<C>::Fr;
    using S = Fp<Fr>;
    constexpr int N = C::N;
    Affine<Fp<C>> P;
    const bool c0_inf = decode_point(c0_xyz, P);
    vk->c0_bad = (!c0_inf && !on_curve(P, K)) ? 1u : 0u;
    vk->c0[0] = P.x;
    vk->c0[1] = P.y;
    const Fp<C> sx = fp_from_mont(P.x), sy = fp_from_mont(P.y);
    for (int i = 0; i < N; i++) { vk->c0_std[i] = sx.l[i]; vk->c0_std[N + i] = sy.l[i]; }
    vk->bad = kzg_vk_prepare(x2_xyz, omega_mont, power, K, vk->g, tab_x2, tab_g2, vk->omega, vk->n_inv, vk->x2_inf) ? 1u : 0u;
    S c[6];
    for (int j = 0; j < 6; j++) {
        for (int i = 0; i < 8; i++) c[j].l[i] = consts[8 * j + i];
        c[j] = fp_to_mont(c[j]);
    }
    vk->k1 = c[0];
    vk->k2 = c[1];
    vk->wr = c[5];
    vk->w8p[0] = vk->w4p[0] = vk->w3p[0] = fp_one<Fr>();
    for (int i = 1; i < 8; i++) vk->w8p[i] = fp_mul(vk->w8p[i - 1], c[4]);
    for (int i = 1; i < 4; i++) vk->w4p[i] = fp_mul(vk->w4p[i - 1], c[3]);
    for (int i = 1; i < 3; i++) vk->w3p[i] = fp_mul(vk->w3p[i - 1], c[2]);
    vk->power = power;
    vk->n_public = n_public;
}

// ---- per proof ------------------------------------------------------------------------------------------------------------------------
// v[0..cnt) -> their inverses, with one fp_inv (Montgomery's trick); pre is scratch of cnt elements
template <class Fr> ZK_DEV void fflonk_batch_inv(Fp<Fr>* v, Fp<Fr>* pre, int cnt) {
    pre[0] = v[0];
    for (int i = 1; i < cnt; i++) pre[i] = fp_mul(pre[i - 1], v[i]);
    Fp<Fr> inv = fp_inv(pre[cnt - 1]);
    for (int i = cnt - 1; i > 0; i--) {
        const Fp<Fr> t = fp_mul(inv, pre[i - 1]);
        inv = fp_mul(inv, v[i]);
        v[i] = t;
    }
    v[0] = inv;
}
// the top bit of a scalar in standard form, which then moves up by one bit: every index is a constant
template <class Fr> ZK_DEV bool fflonk_next_bit(Fp<Fr>& s) {
    const bool b = s.l[7] >> 31;
#pragma unroll
    for (int i = 7; i > 0; i--) s.l[i] = (s.l[i] << 1) | (s.l[i - 1] >> 31);
    s.l[0] <<= 1;
    return b;
}
template <class C> ZK_DEV bool fflonk_point(const uint32_t* xyz, Affine<Fp<C>>& P, bool& fin, const PairingConsts<C>* K) {
    fin = !decode_point(xyz, P);
    return !fin || on_curve(P, K);
}

// proof record: C1 C2 W1 W2 as (x, y, z) (12 Fq) | ql qr qm qo qc s1 s2 s3 a b c z zw t1w t2w (8 words each), standard form;
// pubs: vk.n_public x 8 words. tr (may be null) receives the intermediate values of a proof that passes the input checks.
template <class C> constexpr int fflonk_record_words() { return 12 * C::N + 8 * FFLONK_EVALS; }
// With AGG the check stops before the pairing and hands over its two G1 points, A1 and W2, instead (the aggregated check, kzg_aggregate.cuh; KzgPair:
// kzg_verify.cuh); the code is then FFLONKV_VALID for "the input checks passed". Without it (the default:
// the per-proof kernel) the function is what it was.
template <class C, bool AGG = false>
ZK_PAIR_OP int fflonk_verify_one(const uint32_t* rec, const uint32_t* pubs, const FflonkVkView<C>& V, const PairingConsts<C>* K, FflonkTrace<C>* tr, KzgPair<C>* pair = nullptr) {
    using Fr = typename PairingCfg<C>::Fr;
    using S = Fp<Fr>;
    constexpr int N = C::N;
    const FflonkVk<C>& vk = *V.vk;
    const uint32_t np = vk.n_public;
    Affine<Fp<C>> C1, C2, W1, W2;
    bool fin1, fin2, fin3, w2_fin;
    bool ok = fflonk_point(rec, C1, fin1, K);
    ok = fflonk_point(rec + 3 * N, C2, fin2, K) && ok;
    ok = fflonk_point(rec + 6 * N, W1, fin3, K) && ok;
    ok = fflonk_point(rec + 9 * N, W2, w2_fin, K) && ok;
    if (!ok || vk.c0_bad) return FFLONKV_BAD_POINT;
    for (uint32_t j = 0; j < np; j++)
        if (!public_below_r<C>(pubs + 8 * j)) return FFLONKV_BAD_PUBLIC;
    S ev[FFLONK_EVALS];
    for (int j = 0; j < FFLONK_EVALS; j++) {
        S t;
        for (int i = 0; i < 8; i++) t.l[i] = rec[12 * N + 8 * j + i];
        ev[j] = fp_to_mont(t);
    }
    // challenges (:198-319)
    Keccak256 k;
    keccak_init(k);
    keccak_be(k, vk.c0_std, N); keccak_be(k, vk.c0_std + N, N);
    for (uint32_t j = 0; j < np; j++) keccak_be(k, pubs + 8 * j, 8);
    keccak_point(k, C1);
    const S beta = keccak_challenge<Fr>(k);
    keccak_init(k); keccak_fr(k, beta);
    const S gamma = keccak_challenge<Fr>(k);
    keccak_init(k); keccak_fr(k, gamma); keccak_point(k, C2);
    const S xs = keccak_challenge<Fr>(k);
    keccak_init(k); keccak_fr(k, xs);
    for (int j = 0; j < FFLONK_EVALS; j++) keccak_fr(k, ev[j]);
    const S alpha = keccak_challenge<Fr>(k);
    keccak_init(k); keccak_fr(k, alpha); keccak_point(k, W1);
    const S y = keccak_challenge<Fr>(k);
    // the roots, xi, xi^n, Z_H
    const S one = fp_one<Fr>();
    const S xs2 = fp_sqr(xs), h0 = fp_mul(xs2, xs), h1 = fp_sqr(h0), h2 = fp_mul(h1, xs2), h3 = fp_mul(h2, vk.wr);
    const S xi = fp_mul(fp_sqr(h2), h2), xiw = fp_mul(xi, vk.omega);
    S xin = xi;
    for (uint32_t i = 0; i < vk.power; i++) xin = fp_sqr(xin);
    const S zh = fp_sub(xin, one);
    // every denominator of the Fr part, one inversion: Z_H | S0 (8) S1 (4) S2 (3) S2' (3) | mulH1 mulH2 | xi - w^i (first eight)
    S rt[18], den[FFLONK_FIXED_DENS + 8], pre[FFLONK_FIXED_DENS + 8];
    den[0] = zh;
    S mulH0 = one, mulH1 = one, mulH2 = one;
    {
        // computeLagrangeLiSi (:554-571): den_i = len root_0^(len-2) root_((len-1) i mod len) (y - root_i)
        const S h0_6 = fp_mul(fp_sqr(h1), h1);
        S d8 = fp_add(h0_6, h0_6); d8 = fp_add(d8, d8); d8 = fp_add(d8, d8);
        for (int i = 0; i < 8; i++) {
            rt[i] = fp_mul(h0, vk.w8p[i]);
            const S dy = fp_sub(y, rt[i]);
            mulH0 = fp_mul(mulH0, dy);
            den[1 + i] = fp_mul(fp_mul(d8, fp_mul(h0, vk.w8p[(7 * i) & 7])), dy);
        }
        const S h1_2 = fp_sqr(h1);
        S d4 = fp_add(h1_2, h1_2); d4 = fp_add(d4, d4);
        for (int i = 0; i < 4; i++) {
            rt[8 + i] = fp_mul(h1, vk.w4p[i]);
            const S dy = fp_sub(y, rt[8 + i]);
            mulH1 = fp_mul(mulH1, dy);
            den[9 + i] = fp_mul(fp_mul(d4, fp_mul(h1, vk.w4p[(3 * i) & 3])), dy);
        }
        // computeLagrangeLiS2 (:573-597): den_i = 3 root_0 (xi - xiw) root_(2 i mod 3) (y - root_i), and the same with xi, xiw swapped for S2'
        const S dxi = fp_sub(xi, xiw);
        const S d3a = fp_mul(fp_add(fp_add(h2, h2), h2), dxi), d3b = fp_neg(fp_mul(fp_add(fp_add(h3, h3), h3), dxi));
        for (int i = 0; i < 3; i++) {
            const int c = (2 * i) % 3;
            rt[12 + i] = fp_mul(h2, vk.w3p[i]);
            rt[15 + i] = fp_mul(h3, vk.w3p[i]);
            const S dya = fp_sub(y, rt[12 + i]), dyb = fp_sub(y, rt[15 + i]);
            mulH2 = fp_mul(mulH2, fp_mul(dya, dyb));
            den[13 + i] = fp_mul(fp_mul(d3a, fp_mul(h2, vk.w3p[c])), dya);
            den[16 + i] = fp_mul(fp_mul(d3b, fp_mul(h3, vk.w3p[c])), dyb);
        }
        den[19] = mulH1;
        den[20] = mulH2;
    }
    // L_i(xi) = w^(i-1) Z_H / (n (xi - w^(i-1))) and PI(xi) (:321-356), eight at a time; the first eight share the inversion of the rest
    const S zhn = fp_mul(zh, vk.n_inv);
    S pi = fp_zero<Fr>(), L1 = fp_zero<Fr>(), w = one;
    const uint32_t m = np ? np : 1;
    for (uint32_t at = 0; at < m; at += 8) {
        const uint32_t cnt = m - at < 8 ? m - at : 8;
        S num[8];
        for (uint32_t i = 0; i < cnt; i++) {
            num[i] = fp_mul(w, zhn);
            den[FFLONK_FIXED_DENS + i] = fp_sub(xi, w);
            w = fp_mul(w, vk.omega);
        }
        if (at == 0) fflonk_batch_inv(den, pre, FFLONK_FIXED_DENS + (int)cnt);
        else fflonk_batch_inv(den + FFLONK_FIXED_DENS, pre, (int)cnt);
        for (uint32_t i = 0; i < cnt; i++) {
            const S L = fp_mul(num[i], den[FFLONK_FIXED_DENS + i]);
            if (at + i == 0) L1 = L;
            if (at + i < np) {
                S x;
                for (int q = 0; q < 8; q++) x.l[q] = pubs[8 * (at + i) + q];
                pi = fp_sub(pi, fp_mul(fp_to_mont(x), L));
            }
        }
    }
    const S invzh = den[0];
    const S ql = ev[0], qr = ev[1], qm = ev[2], qo = ev[3], qc = ev[4], s1 = ev[5], s2 = ev[6], s3 = ev[7], a = ev[8], b = ev[9], c = ev[10], z = ev[11], zw = ev[12],
            t1w = ev[13], t2w = ev[14];
    // r0 (:358-388): sum_i C0(S0_i) L_i(y), C0(h) = ql + qr h + qo h^2 + qm h^3 + qc h^4 + s1 h^5 + s2 h^6 + s3 h^7
    const S y2 = fp_sqr(y), y3 = fp_mul(y2, y), y4 = fp_sqr(y2);
    S r0 = fp_zero<Fr>();
    for (int i = 0; i < 8; i++) {
        const S h = rt[i];
        S v = s3;
        v = fp_add(fp_mul(v, h), s2); v = fp_add(fp_mul(v, h), s1); v = fp_add(fp_mul(v, h), qc); v = fp_add(fp_mul(v, h), qm);
        v = fp_add(fp_mul(v, h), qo); v = fp_add(fp_mul(v, h), qr); v = fp_add(fp_mul(v, h), ql);
        r0 = fp_add(r0, fp_mul(v, den[1 + i]));
    }
    r0 = fp_mul(r0, fp_sub(fp_sqr(y4), xi));
    // r1 (:390-426): C1(h) = a + b h + c h^2 + T0 h^3, T0 = (ql a + qr b + qm a b + qo c + qc + PI) / Z_H
    S t0 = fp_add(fp_add(fp_mul(ql, a), fp_mul(qr, b)), fp_add(fp_mul(fp_mul(qm, a), b), fp_mul(qo, c)));
    t0 = fp_mul(fp_add(fp_add(t0, qc), pi), invzh);
    S r1 = fp_zero<Fr>();
    for (int i = 0; i < 4; i++) {
        const S h = rt[8 + i];
        const S v = fp_add(fp_mul(fp_add(fp_mul(fp_add(fp_mul(t0, h), c), h), b), h), a);
        r1 = fp_add(r1, fp_mul(v, den[9 + i]));
    }
    r1 = fp_mul(r1, fp_sub(y4, xi));
    // r2 (:428-486): C2(h) = z + T1 h + T2 h^2 on S2, zw + t1w h + t2w h^2 on S2'
    const S t1 = fp_mul(fp_mul(fp_sub(z, one), L1), invzh);
    const S bxi = fp_mul(beta, xi);
    const S t21 = fp_mul(fp_mul(fp_mul(fp_add(fp_add(a, bxi), gamma), fp_add(fp_add(b, fp_mul(bxi, vk.k1)), gamma)), fp_add(fp_add(c, fp_mul(bxi, vk.k2)), gamma)), z);
    const S t22 = fp_mul(fp_mul(fp_mul(fp_add(fp_add(a, fp_mul(beta, s1)), gamma), fp_add(fp_add(b, fp_mul(beta, s2)), gamma)), fp_add(fp_add(c, fp_mul(beta, s3)), gamma)), zw);
    const S t2 = fp_mul(fp_sub(t21, t22), invzh);
    S r2 = fp_zero<Fr>();
    for (int i = 0; i < 3; i++) {
        const S ha = rt[12 + i], hb = rt[15 + i];
        r2 = fp_add(r2, fp_mul(fp_add(fp_mul(fp_add(fp_mul(t2, ha), t1), ha), z), den[13 + i]));
        r2 = fp_add(r2, fp_mul(fp_add(fp_mul(fp_add(fp_mul(t2w, hb), t1w), hb), zw), den[16 + i]));
    }
    r2 = fp_mul(r2, fp_add(fp_sub(fp_sqr(y3), fp_mul(fp_add(xi, xiw), y3)), fp_mul(xi, xiw)));
    // the scalars of F, E, J (:488-537)
    const S amul = fp_mul(alpha, mulH0);
    const S q1 = fp_mul(amul, den[19]), q2 = fp_mul(fp_mul(amul, alpha), den[20]);
    const S e = fp_add(r0, fp_add(fp_mul(r1, q1), fp_mul(r2, q2)));
    // A1 = C0 + q1 C1 + q2 C2 - e G - mulH0 W1 + y W2: Straus over five bases, then C0
    S sc1 = fp_from_mont(q1), sc2 = fp_from_mont(q2), scg = fp_from_mont(fp_neg(e)), scw1 = fp_from_mont(fp_neg(mulH0)), scw2 = fp_from_mont(y);
    const Affine<Fp<C>> G{vk.g[0], vk.g[1]};
    XYZZ<Fp<C>> acc;
    pt_set_inf(acc);
    for (int bit = 255; bit >= 0; bit--) {
        acc = pt_dbl(acc);
        if (fflonk_next_bit(sc1)) pt_madd(acc, C1);
        if (fflonk_next_bit(sc2)) pt_madd(acc, C2);
        if (fflonk_next_bit(scg)) pt_madd(acc, G);
        if (fflonk_next_bit(scw1)) pt_madd(acc, W1);
        if (fflonk_next_bit(scw2)) pt_madd(acc, W2);
    }
    pt_madd(acc, Affine<Fp<C>>{vk.c0[0], vk.c0[1]});
    Fp<C> ax, ay;
    const bool a_fin = xyzz_to_affine(acc, ax, ay);
    if (tr) {
        const S t[8] = {beta, gamma, xi, alpha, y, r0, r1, r2};
        for (int j = 0; j < 8; j++) {
            const S s = fp_from_mont(t[j]);
            for (int i = 0; i < 8; i++) tr->fr[j][i] = s.l[i];
        }
        const Fp<C> p[4] = {fp_from_mont(ax), fp_from_mont(ay), fp_from_mont(W2.x), fp_from_mont(W2.y)};
        for (int i = 0; i < N; i++) { tr->a1[i] = p[0].l[i]; tr->a1[N + i] = p[1].l[i]; tr->b1[i] = p[2].l[i]; tr->b1[N + i] = p[3].l[i]; }
    }
    if constexpr (AGG) {
        *pair = KzgPair<C>{ax, ay, W2.x, W2.y, a_fin, w2_fin};
        return FFLONKV_VALID;
    } else {
        // e(-A1, [1]_2) e(W2, X_2) == 1 (:539-551); pairs are passed as (-px, py)
        const FixedPair<C> f0{V.tab_g2, fp_neg(ax), fp_neg(ay), a_fin};
        const FixedPair<C> f1{V.tab_x2, fp_neg(W2.x), W2.y, w2_fin && !vk.x2_inf};
        Affine<Fp2<C>> none;
        f_set_zero(none.x);
        f_set_zero(none.y);
        const Fp12<C> f = miller_multi(none, ax, ay, false, f0, f1, K);
        return f12_is_one(final_exp(f, K)) ? FFLONKV_VALID : FFLONKV_INVALID;
    }
}

}  // namespace zkmi
