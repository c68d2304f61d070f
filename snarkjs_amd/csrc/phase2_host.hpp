// snarkjs_amd/csrc/phase2_host.hpp — the host side of a Groth16 phase-2 contribution: the reference's deterministic generator and what it
// draws from it, restated on host_field.hpp. O(1) work per contribution, no device.
//   ChaCha            ffjavascript's ChaCha (min.js: 20 rounds, the 128-bit block counter in words 12 - 15, the eight seed words in 4 - 11)
//   field_from_rng    F.fromRng: n64 nextU64 words little-endian, masked to the modulus' bit length, drawn again while >= p. The WASM field keeps these raw
//                     bytes as the element: the integer drawn IS the Montgomery representation.
//   point_from_rng    G.fromRng: x = F.fromRng, sign = nextBool until x^3 + b is a square; y = its root, negated when sign != isNegative(y); times the
//                     cofactor where the reference's curve record has one (BN254 G2, BLS12-381 G1 and G2)
// Which of the two roots the square root finds does not matter: isNegative picks the one that is kept.
#pragma once
#include "host_field.hpp"

namespace zkmi {
namespace phase2 {

struct ChaCha {
    uint32_t state[16], buff[16];
    int idx = 16;
    explicit ChaCha(const uint32_t seed[8]) {
        state[0] = 0x61707865u; state[1] = 0x3320646eu; state[2] = 0x79622d32u; state[3] = 0x6b206574u;
        for (int i = 0; i < 8; i++) state[4 + i] = seed[i];
        for (int i = 12; i < 16; i++) state[i] = 0;
    }
    static uint32_t rotl(uint32_t v, int s) { return (v << s) | (v >> (32 - s)); }
    static void quarter(uint32_t* x, int a, int b, int c, int d) {
        x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 16);
        x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 12);
        x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 8);
        x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 7);
    }
    void update() {
        for (int i = 0; i < 16; i++) buff[i] = state[i];
        for (int r = 0; r < 10; r++) {
            quarter(buff, 0, 4, 8, 12); quarter(buff, 1, 5, 9, 13); quarter(buff, 2, 6, 10, 14); quarter(buff, 3, 7, 11, 15);
            quarter(buff, 0, 5, 10, 15); quarter(buff, 1, 6, 11, 12); quarter(buff, 2, 7, 8, 13); quarter(buff, 3, 4, 9, 14);
        }
        for (int i = 0; i < 16; i++) buff[i] += state[i];
        idx = 0;
        for (int i = 12; i < 16 && ++state[i] == 0; i++) {}
    }
    uint32_t next_u32() { if (idx == 16) update(); return buff[idx++]; }
    uint64_t next_u64() { const uint64_t hi = next_u32(); return (hi << 32) | next_u32(); }
    bool next_bool() { return (next_u32() & 1u) != 0; }
};

template <int L> int bit_length(const uint64_t (&p)[L]) {
    for (int i = 64 * L - 1; i >= 0; i--) if ((p[i / 64] >> (i % 64)) & 1) return i + 1;
    return 0;
}

template <int L> host::HFp<L> field_from_rng(const host::HField<L>& F, ChaCha& rng) {
    const int bits = bit_length<L>(F.p);
    host::HFp<L> a;
    do {
        for (int i = 0; i < L; i++) a.v[i] = rng.next_u64();
        for (int i = 0; i < L; i++) {
            const int keep = bits - 64 * i;
            if (keep <= 0) a.v[i] = 0; else if (keep < 64) a.v[i] &= (((uint64_t)1 << keep) - 1);
        }
    } while (host::HField<L>::cmp(a.v, F.p) >= 0);
    return a;
}
template <int L> host::HFp<L> elem_from_rng(const host::HField<L>& F, ChaCha& rng) { return field_from_rng(F, rng); }
template <int L> host::HFp2<L> elem_from_rng(const host::HField2<L>& F2, ChaCha& rng) {
    host::HFp2<L> r;
    r.c0 = field_from_rng(F2.F, rng); r.c1 = field_from_rng(F2.F, rng);
    return r;
}

// (p + num) / 4 for num = 1 | -3: the exponents of the square roots below (p = 3 mod 4 on both curves)
template <int L> void quarter_exp(const host::HField<L>& F, int num, uint64_t (&e)[L]) {
    for (int i = 0; i < L; i++) e[i] = F.p[i];
    if (num > 0) e[0] += 1; else e[0] -= 3;                                      // p = ...11 in binary: no carry or borrow leaves the low word
    for (int i = 0; i < L; i++) e[i] = (e[i] >> 2) | (i + 1 < L ? e[i + 1] << 62 : 0);
}
template <class FT> typename FT::E pow_words(const FT& F, const typename FT::E& a, const uint64_t* e, int ne) {
    typename FT::E r = F.One(), b = a;
    for (int i = 0; i < 64 * ne; i++) { if ((e[i / 64] >> (i % 64)) & 1) r = F.mul(r, b); b = F.sqr(b); }
    return r;
}

// square roots; false when `a` is not a square
template <int L> bool elem_sqrt(const host::HField<L>& F, const host::HFp<L>& a, host::HFp<L>& r) {
    uint64_t e[L];
    quarter_exp(F, 1, e);
    r = F.pow(a, e, L);
    return F.sqr(r) == a;
}
// Fq2 = Fq[u] / (u^2 + 1) (Adj, Rodriguez-Henriquez: "Square root computation over even extension fields", Alg. 9, as gconv.cuh on the device)
template <int L> bool elem_sqrt(const host::HField2<L>& F2, const host::HFp2<L>& a, host::HFp2<L>& r) {
    const host::HField<L>& F = F2.F;
    uint64_t e[L];
    quarter_exp(F, -3, e);
    const host::HFp2<L> a1 = pow_words(F2, a, e, L), x0 = F2.mul(a1, a), alpha = F2.mul(a1, x0);
    if (alpha.c1.is_zero() && alpha.c0 == F.neg(F.One())) r = host::HFp2<L>{F.neg(x0.c1), x0.c0};        // u x0
    else {
        uint64_t h[L];                                                           // (p - 1) / 2
        for (int i = 0; i < L; i++) h[i] = (F.p[i] >> 1) | (i + 1 < L ? F.p[i + 1] << 63 : 0);
        r = F2.mul(pow_words(F2, F2.add(F2.One(), alpha), h, L), x0);
    }
    return F2.sqr(r) == a;
}

// the reference's isNegative: the normal form exceeds (p - 1) / 2; an Fq2 element by c1, or by c0 when c1 is zero
template <int L> bool elem_is_negative(const host::HField<L>& F, const host::HFp<L>& a) {
    const host::HFp<L> n = F.from_mont(a);
    uint64_t h[L];
    for (int i = 0; i < L; i++) h[i] = (F.p[i] >> 1) | (i + 1 < L ? F.p[i + 1] << 63 : 0);
    return host::HField<L>::cmp(n.v, h) > 0;
}
template <int L> bool elem_is_negative(const host::HField2<L>& F2, const host::HFp2<L>& a) { return a.c1.is_zero() ? elem_is_negative(F2.F, a.c0) : elem_is_negative(F2.F, a.c1); }

// G.fromRng over the field FT with curve constant b; cofactor: plain little-endian bytes (nbits = 0: none)
template <class FT> typename host::HCurve<FT>::P point_from_rng(const FT& F, const typename FT::E& b, const uint8_t* cofactor, int cofactor_bits, ChaCha& rng) {
    typename FT::E x, y, rhs;
    bool sign;
    do {
        x = elem_from_rng(F, rng);
        sign = rng.next_bool();
        rhs = F.add(F.mul(F.sqr(x), x), b);
    } while (!elem_sqrt(F, rhs, y));
    if (sign != elem_is_negative(F, y)) y = F.neg(y);
    host::HCurve<FT> cv{F};
    typename host::HCurve<FT>::P p = cv.from_affine(x, y);
    return cofactor_bits ? cv.mul_bits(p, cofactor, cofactor_bits) : p;
}

}  // namespace phase2
}  // namespace zkmi
