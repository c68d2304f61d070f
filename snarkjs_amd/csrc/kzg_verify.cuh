// snarkjs_amd/csrc/kzg_verify.cuh — what the per-proof PLONK and FFLONK checks (plonk_verify.cuh, fflonk_verify.cuh) share, gfx950.
//
// The generators of G1 and G2, Keccak-256 and the Fiat-Shamir transcript's encoding (src/Keccak256Transcript.js: points as x | y big-endian
// standard form, the point at infinity as zero bytes, scalars 32 bytes big-endian, challenge = digest mod r), XYZZ to affine, and the part of a
// key's preparation that both protocols do alike (kzg_vk_prepare).
//
// Like pairing.cuh this is __device__ code that also compiles for the host (tools/*_verify_hosttest.hip, __device__ defined away).
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

// ---- the transcript's items and challenges; XYZZ to affine ----------------------------------------------------------------------------
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

// The two G1 points a per-proof check ends in, e(-P, T0) e(Q, T1) == 1 with T0, T1 fixed per key, as the aggregated check takes them over
// (kzg_aggregate.cuh): affine, Montgomery; *_fin off for the point at infinity.
template <class C> struct KzgPair {
    Fp<C> px, py, qx, qy;
    bool p_fin, q_fin;
};

// ---- per verifying key: the generators to Montgomery form (g1: x, y), the line tables of the G2 generator and of X_2, omega = Fr.w[power]
// (passed in Montgomery form), 1/n for n = 2^power, whether X_2 is the point at infinity. True when X_2 is not on its curve. One lane, once.
template <class C>
ZK_DEV bool kzg_vk_prepare(const uint32_t* x2_xyz, const uint32_t* omega_mont, uint32_t power, const PairingConsts<C>* K, Fp<C>* g1, Line<C>* tab_x2, Line<C>* tab_g2,
                           Fp<typename PairingCfg<C>::Fr>& omega, Fp<typename PairingCfg<C>::Fr>& n_inv, uint32_t& x2_is_inf) {
    using Fr = typename PairingCfg<C>::Fr;
    constexpr int N = C::N;
    Fp<C> gx, gy;
    Affine<Fp2<C>> G;
    for (int i = 0; i < N; i++) {
        gx.l[i] = PlonkGen<C>::g1(i); gy.l[i] = PlonkGen<C>::g1(N + i);
        G.x.c0.l[i] = PlonkGen<C>::g2(i); G.x.c1.l[i] = PlonkGen<C>::g2(N + i);
        G.y.c0.l[i] = PlonkGen<C>::g2(2 * N + i); G.y.c1.l[i] = PlonkGen<C>::g2(3 * N + i);
    }
    g1[0] = fp_to_mont(gx);
    g1[1] = fp_to_mont(gy);
    G.x = f_to_mont_any(G.x);
    G.y = f_to_mont_any(G.y);
    g2_line_table(G, tab_g2, K);
    Affine<Fp2<C>> X2;
    const bool x2_inf = decode_point(x2_xyz, X2);
    bool bad = false;
    if (!x2_inf) {
        bad = !on_curve(X2, K);
        g2_line_table(X2, tab_x2, K);
    }
    Fp<Fr> w, n = fp_zero<Fr>();
    for (int i = 0; i < 8; i++) {
        w.l[i] = omega_mont[i];
        if ((uint32_t)i == (power >> 5)) n.l[i] = 1u << (power & 31);
    }
    omega = w;
    n_inv = fp_inv(fp_to_mont(n));
    x2_is_inf = x2_inf ? 1u : 0u;
    return bad;
}

}  // namespace zkmi
