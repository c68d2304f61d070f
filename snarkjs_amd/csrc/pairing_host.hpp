// snarkjs_amd/csrc/pairing_host.hpp — host derivation of the pairing constants of pairing.cuh from the field constants of field.cuh.
//
// gamma_{1,k} = xi^(k (p-1)/6) (Fq2), gamma_{2,k} = gamma_{1,k}^(p+1) = gamma_{1,k} * conj(gamma_{1,k}) (in Fq), the twist's b (b/xi for the
// D-type BN254 twist, b*xi for the M-type BLS12-381 twist), and the hard part (p^4 - p^2 + 1)/r of the final exponent, computed by exact
// division modulo 2^1536 (r is odd: q = N * r^-1 mod 2^1536 is the quotient because r divides N and q < 2^1536). Nothing is typed in.
#pragma once
#include <string.h>
#include "host_field.hpp"
#include "pairing.cuh"

namespace zkmi {

namespace pairing_host_detail {
constexpr int W = 48;                                     // 1536-bit arithmetic modulo 2^1536
inline void mul_lo(const uint32_t* a, const uint32_t* b, uint32_t* out) {
    uint32_t t[W] = {0};
    for (int i = 0; i < W; i++) {
        uint64_t c = 0;
        for (int j = 0; i + j < W; j++) {
            c += (uint64_t)a[i] * b[j] + t[i + j];
            t[i + j] = (uint32_t)c;
            c >>= 32;
        }
    }
    memcpy(out, t, sizeof t);
}
inline void sub_lo(const uint32_t* a, const uint32_t* b, uint32_t* out) {
    uint64_t bw = 0;
    for (int i = 0; i < W; i++) { uint64_t d = (uint64_t)a[i] - b[i] - bw; out[i] = (uint32_t)d; bw = (d >> 63) & 1; }
}
inline void add_small(uint32_t* a, uint32_t k) {
    uint64_t c = k;
    for (int i = 0; i < W && c; i++) { c += a[i]; a[i] = (uint32_t)c; c >>= 32; }
}
}  // namespace pairing_host_detail

template <class C> inline void pairing_consts_host(PairingConsts<C>& K) {
    using namespace pairing_host_detail;
    constexpr int L = C::N / 2;
    using Cfg = PairingCfg<C>;
    using Fr = typename Cfg::Fr;
    host::HField2<L> F2;
    F2.F = host::HField<L>::template from_cfg<C>();
    auto& F = F2.F;
    auto to_dev = [](const host::HFp<L>& a, Fp<C>& o) {
        for (int i = 0; i < L; i++) { o.l[2 * i] = (uint32_t)a.v[i]; o.l[2 * i + 1] = (uint32_t)(a.v[i] >> 32); }
    };
    auto to_dev2 = [&](const host::HFp2<L>& a, Fp2<C>& o) { to_dev(a.c0, o.c0); to_dev(a.c1, o.c1); };
    const host::HFp2<L> xi{F.from_u64(Cfg::XI_S), F.from_u64(1)};
    // e = (p - 1)/6 by long division
    uint64_t e[L];
    {
        uint32_t w[C::N];
        uint64_t rem = 0;
        for (int i = C::N - 1; i >= 0; i--) {
            uint64_t cur = (rem << 32) | (i == 0 ? C::p(0) - 1 : C::p(i));
            w[i] = (uint32_t)(cur / 6);
            rem = cur % 6;
        }
        for (int i = 0; i < L; i++) e[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
    }
    // xi^e by square-and-multiply
    host::HFp2<L> g = F2.One(), b = xi;
    for (int i = 0; i < 64 * L; i++) { if ((e[i / 64] >> (i % 64)) & 1) g = F2.mul(g, b); b = F2.sqr(b); }
    host::HFp2<L> gk = F2.One();
    for (int k = 0; k < 6; k++) {
        to_dev2(gk, K.g1[k]);
        to_dev2(F2.mul(gk, host::HFp2<L>{gk.c0, F.neg(gk.c1)}), K.g2[k]);
        gk = F2.mul(gk, g);
    }
    const host::HFp<L> b1 = F.from_u64(Cfg::B);
    to_dev(b1, K.b);
    const host::HFp2<L> bb{b1, F.zero()};
    to_dev2(Cfg::D_TWIST ? F2.mul(bb, F2.inv(xi)) : F2.mul(bb, xi), K.twist_b);
    // hard = (p^4 - p^2 + 1) / r
    uint32_t p[W] = {0}, r[W] = {0}, p2[W], p4[W], n[W], rinv[W], t[W], two[W] = {0};
    for (int i = 0; i < C::N; i++) p[i] = C::p(i);
    for (int i = 0; i < 8; i++) r[i] = Fr::p(i);
    mul_lo(p, p, p2);
    mul_lo(p2, p2, p4);
    sub_lo(p4, p2, n);
    add_small(n, 1);
    // r^-1 mod 2^1536 by Newton: x <- x (2 - r x), doubling the correct bits from 1 (r odd: x = 1 is right mod 2)
    memset(rinv, 0, sizeof rinv);
    rinv[0] = 1;
    two[0] = 2;
    for (int it = 0; it < 11; it++) {
        mul_lo(r, rinv, t);
        sub_lo(two, t, t);
        mul_lo(rinv, t, rinv);
    }
    mul_lo(n, rinv, K.hard);
    K.hard_bits = 0;
    for (int i = W * 32 - 1; i >= 0; i--)
        if ((K.hard[i >> 5] >> (i & 31)) & 1) { K.hard_bits = (uint32_t)i + 1; break; }
}

}  // namespace zkmi
