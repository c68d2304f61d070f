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
#include "pairing.cuh"

namespace zkmi {

// ---- the generators of G1 and G2 (standard form, little-endian words; G2: x.c0 x.c1 y.c0 y.c1) — ffjavascript's curve.G1.g / curve.G2.g -------
template <class C> struct PlonkGen;
template <> struct PlonkGen<Bn254Fq> {
    ZK_HD static constexpr uint32_t g1(int i) {
        constexpr uint32_t v[16] = {1, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0};
        return v[i];
    }
    ZK_HD static constexpr uint32_t g2(int i) {
        constexpr uint32_t v[32] = {0xd992f6edu, 0x46debd5cu, 0xf75edaddu, 0x674322d4u, 0x5e5c4479u, 0x426a0066u, 0x121f1e76u, 0x1800deefu,
                                    0xaef312c2u, 0x97e485b7u, 0x35a9e712u, 0xf1aa4933u, 0x31fb5d25u, 0x7260bfb7u, 0x920d483au, 0x198e9393u,
                                    0x66fa7daau, 0x4ce6cc01u, 0x0c43d37bu, 0xe3d1e769u, 0x8dcb408fu, 0x4aab7180u, 0xdb8c6debu, 0x12c85ea5u,
                                    0xd122975bu, 0x55acdadcu, 0x70b38ef3u, 0xbc4b3133u, 0x690c3395u, 0xec9e99adu, 0x585ff075u, 0x090689d0u};
        return v[i];
    }
};
template <> struct PlonkGen<Bls12381Fq> {
    ZK_HD static constexpr uint32_t g1(int i) {
        constexpr uint32_t v[24] = {0xdb22c6bbu, 0xfb3af00au, 0xf97a1aefu, 0x6c55e83fu, 0x171bac58u, 0xa14e3a3fu, 0x9774b905u, 0xc3688c4fu, 0x4fa9ac0fu, 0x2695638cu, 0x3197d794u, 0x17f1d3a7u,
                                    0x46c5e7e1u, 0x0caa2329u, 0xa2888ae4u, 0xd03cc744u, 0x2c04b3edu, 0x00db18cbu, 0xd5d00af6u, 0xfcf5e095u, 0x741d8ae4u, 0xa09e30edu, 0xe3aaa0f1u, 0x08b3f481u};
        return v[i];
    }
    ZK_HD static constexpr uint32_t g2(int i) {
        constexpr uint32_t v[48] = {0xc121bdb8u, 0xd48056c8u, 0xa805bbefu, 0x0bac0326u, 0x7ae3d177u, 0xb4510b64u, 0xfa403b02u, 0xc6e47ad4u, 0x2dc51051u, 0x26080527u, 0xf08f0a91u, 0x024aa2b2u,
                                    0x5d042b7eu, 0xe5ac7d05u, 0x13945d57u, 0x334cf112u, 0xdc7f5049u, 0xb5da61bbu, 0x9920b61au, 0x596bd0d0u, 0x88274f65u, 0x7dacd3a0u, 0x52719f60u, 0x13e02b60u,
                                    0x08b82801u, 0xe1935486u, 0x3baca289u, 0x923ac9ccu, 0x5160d12cu, 0x6d429a69u, 0x8cbdd3a7u, 0xadfd9baau, 0xda2e351au, 0x8cc9cdc6u, 0x727d6e11u, 0x0ce5d527u,
                                    0xf05f79beu, 0xaaa9075fu, 0x5cec1da1u, 0x3f370d27u, 0x572e99abu, 0x267492abu, 0x85a763afu, 0xcb3e287eu, 0x2bc28b99u, 0x32acd2b0u, 0x2ea734ccu, 0x0606c4a0u};
        return v[i];
    }
};

// ---- Keccak-256 with the original 0x01 padding (@noble/hashes keccak_256), rate 136 bytes = 17 lanes ------------------------------------
struct Keccak256 {
    uint64_t st[25];
    uint32_t pos;                 // next 8-byte lane of the rate
};
inline __device__ __noinline__ void keccak_f1600(uint64_t* st) {
    constexpr uint64_t RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
                                 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
                                 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
                                 0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    constexpr int ROT[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
    constexpr int PIL[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};
    uint64_t a[25];
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] = st[i];
    for (int round = 0; round < 24; round++) {
        uint64_t bc[5];
#pragma unroll
        for (int i = 0; i < 5; i++) bc[i] = a[i] ^ a[i + 5] ^ a[i + 10] ^ a[i + 15] ^ a[i + 20];
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const uint64_t t = bc[(i + 4) % 5] ^ ((bc[(i + 1) % 5] << 1) | (bc[(i + 1) % 5] >> 63));
#pragma unroll
            for (int j = 0; j < 25; j += 5) a[j + i] ^= t;
        }
        uint64_t t = a[1];
#pragma unroll
        for (int i = 0; i < 24; i++) {
            const uint64_t b = a[PIL[i]];
            a[PIL[i]] = (t << ROT[i]) | (t >> (64 - ROT[i]));
            t = b;
        }
#pragma unroll
        for (int j = 0; j < 25; j += 5) {
#pragma unroll
            for (int i = 0; i < 5; i++) bc[i] = a[j + i];
#pragma unroll
            for (int i = 0; i < 5; i++) a[j + i] ^= (~bc[(i + 1) % 5]) & bc[(i + 2) % 5];
        }
        a[0] ^= RC[round];
    }
#pragma unroll
    for (int i = 0; i < 25; i++) st[i] = a[i];
}
ZK_DEV void keccak_init(Keccak256& k) {
    for (int i = 0; i < 25; i++) k.st[i] = 0;
    k.pos = 0;
}
ZK_DEV void keccak_lane(Keccak256& k, uint64_t w) {
    k.st[k.pos++] ^= w;
    if (k.pos == 17) { keccak_f1600(k.st); k.pos = 0; }
}
// the big-endian bytes of a value of nw (even) little-endian words; every item of the transcript is a whole number of lanes
ZK_DEV void keccak_be(Keccak256& k, const uint32_t* w, int nw) {
    for (int i = nw - 2; i >= 0; i -= 2) keccak_lane(k, __builtin_bswap64(((uint64_t)w[i + 1] << 32) | w[i]));
}
// pads a lane-aligned message and writes the digest, read as a big-endian integer, as 8 little-endian words
ZK_DEV void keccak_finish(Keccak256& k, uint32_t* d) {
    k.st[k.pos] ^= 0x01ull;
    k.st[16] ^= 0x8000000000000000ull;
    keccak_f1600(k.st);
    for (int j = 0; j < 4; j++) {
        const uint64_t v = __builtin_bswap64(k.st[3 - j]);
        d[2 * j] = (uint32_t)v;
        d[2 * j + 1] = (uint32_t)(v >> 32);
    }
}

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
    Fp<C> gx, gy;
    Affine<Fp2<C>> G;
    for (int i = 0; i < N; i++) {
        gx.l[i] = PlonkGen<C>::g1(i); gy.l[i] = PlonkGen<C>::g1(N + i);
        G.x.c0.l[i] = PlonkGen<C>::g2(i); G.x.c1.l[i] = PlonkGen<C>::g2(N + i);
        G.y.c0.l[i] = PlonkGen<C>::g2(2 * N + i); G.y.c1.l[i] = PlonkGen<C>::g2(3 * N + i);
    }
    vk->base[8][0] = fp_to_mont(gx);
    vk->base[8][1] = fp_to_mont(gy);
    G.x = f_to_mont_any(G.x);
    G.y = f_to_mont_any(G.y);
    g2_line_table(G, tab_g2, K);
    Affine<Fp2<C>> X2;
    const bool x2_inf = decode_point(x2_xyz, X2);
    if (!x2_inf) {
        if (!on_curve(X2, K)) bad = 1;
        g2_line_table(X2, tab_x2, K);
    }
    S a, b, w, n = fp_zero<typename PairingCfg<C>::Fr>();
    for (int i = 0; i < 8; i++) {
        a.l[i] = k1[i]; b.l[i] = k2[i]; w.l[i] = omega_mont[i];
        if ((uint32_t)i == (power >> 5)) n.l[i] = 1u << (power & 31);
    }
    vk->k1 = fp_to_mont(a);
    vk->k2 = fp_to_mont(b);
    vk->omega = w;
    vk->n_inv = fp_inv(fp_to_mont(n));
    vk->power = power;
    vk->n_public = n_public;
    vk->x2_inf = x2_inf ? 1u : 0u;
    vk->bad = bad;
}

// ---- per proof ------------------------------------------------------------------------------------------------------------------------
template <class Fr> ZK_DEV void keccak_fr(Keccak256& k, const Fp<Fr>& mont) {
    const Fp<Fr> s = fp_from_mont(mont);
    keccak_be(k, s.l, 8);
}
template <class C> ZK_DEV void keccak_point(Keccak256& k, const Affine<Fp<C>>& P) {      // infinity is all-zero in either form
    const Fp<C> x = fp_from_mont(P.x), y = fp_from_mont(P.y);
    keccak_be(k, x.l, C::N);
    keccak_be(k, y.l, C::N);
}
template <class Fr> ZK_DEV Fp<Fr> keccak_challenge(Keccak256& k) {
    Fp<Fr> d;
    keccak_finish(k, d.l);
    return fp_to_mont(d);                      // a value below 2^256 comes out reduced
}
// to affine; false (and zero coordinates) for the point at infinity
template <class C> ZK_DEV bool xyzz_to_affine(const XYZZ<Fp<C>>& p, Fp<C>& x, Fp<C>& y) {
    x = fp_zero<C>();
    y = fp_zero<C>();
    if (pt_is_inf(p)) return false;
    const Fp<C> i = fp_inv(fp_mul(p.ZZ, p.ZZZ));
    x = fp_mul(p.X, fp_mul(i, p.ZZZ));
    y = fp_mul(p.Y, fp_mul(i, p.ZZ));
    return true;
}

// proof record: A B C Z T1 T2 T3 Wxi Wxiw as (x, y, z) (27 Fq) | eval_a eval_b eval_c eval_s1 eval_s2 eval_zw (8 words each), standard form;
// pubs: vk.n_public x 8 words. tr (may be null) receives the intermediate values of a proof that passes the input checks.
template <class C> constexpr int plonk_record_words() { return 27 * C::N + 48; }
template <class C> ZK_PAIR_OP int plonk_verify_one(const uint32_t* rec, const uint32_t* pubs, const PlonkVkView<C>& V, const PairingConsts<C>* K, PlonkTrace<C>* tr) {
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
    // e(-A1, X_2) e(B1, [1]_2) == 1 (:405-421); pairs are passed as (-px, py)
    const FixedPair<C> f0{V.tab_x2, fp_neg(ax), fp_neg(ay), a_fin && !vk.x2_inf};
    const FixedPair<C> f1{V.tab_g2, fp_neg(bx), by, b_fin};
    Affine<Fp2<C>> none;
    f_set_zero(none.x);
    f_set_zero(none.y);
    const Fp12<C> f = miller_multi(none, ax, ay, false, f0, f1, K);
    return f12_is_one(final_exp(f, K)) ? PLONKV_VALID : PLONKV_INVALID;
}

}  // namespace zkmi
