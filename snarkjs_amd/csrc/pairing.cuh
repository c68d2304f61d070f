// snarkjs_amd/csrc/pairing.cuh — optimal ate pairing and the per-proof Groth16 check for BN254 and BLS12-381, gfx950.
//
// Replaces curve.pairingEq of ffjavascript / wasmcurves (reference src/groth16_verify.js:66-74) on the device, one proof per lane.
// Restated after oracle/groth16_verify_oracle.py, which is pinned to the reference's own accept / reject verdicts.
//
// Tower:      Fq2 = Fq[u]/(u^2 + 1) (curve.cuh), Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v); xi = 9 + u (BN254), 1 + u (BLS12-381).
//             The Fq2 coefficient of w^k (k = 2i + j) is Fp12.c<j>.c<i>; with u = w^6 - s (xi = s + u) it maps onto the oracle's
//             w-basis Fq[w]/(w^12 - 2s w^6 + s^2 + 1) as a + b u -> (a - s b) w^k + b w^(k+6).
// Twists:     BN254 D-type (y^2 = x^3 + 3/xi), BLS12-381 M-type (y^2 = x^3 + 4 xi), exactly as the oracle.
// G2 steps:   Jacobian T = (X, Y, Z) — no inversion inside the loop. Every line is the oracle's affine line times a factor in Fq2 (the
//             doubling line times 2 Y Z^3, the addition line times H Z); such a factor lies in a proper subfield and is removed by the
//             final exponentiation, so the reduced values equal the oracle's bit for bit.
// Loop:       binary, MSB first, the oracle's scalar: BN254 6x + 2 (65 bits) followed by the two Frobenius additions (Q1, -Q2);
//             BLS12-381 |x| = 0xd201000000010000. The BLS12-381 x is negative; like the oracle (and the reference, whose pairingEq
//             compares a product with 1) no conjugation is applied: every value is the inverse of the signed-x pairing, alike.
// Final exp:  easy part f^((p^6 - 1)(p^2 + 1)) by conjugation, one inversion and the p^2-Frobenius; hard part (p^4 - p^2 + 1)/r by plain
//             square-and-multiply over its bits. The chain computes the exact exponent (p^12 - 1)/r: the multiple is m = 1.
// Frobenius constants gamma_{n,k} = xi^(k (p^n - 1)/6) and the hard exponent are derived on the host from the field constants
// (pairing_host.hpp) and read from memory by every lane.
//
// Degenerate inputs: a point on the curve outside the subgroup can make T = +-Q at some addition step. The step then yields Z = 0 and the
// lines that follow are degenerate; nothing divides, so the lane finishes and its verdict is whatever the final value says (in practice
// "invalid"). The reference's affine formulas take a different path there; agreement on such constructed inputs is not claimed.
//
// Everything here is __device__ code that also compiles for the host (tools/pairing_hosttest.hip compiles it with ZKMI_MUL_VARIANT 1
// and __device__ defined away), which is how it is checked against the oracle without a GPU.
#pragma once
#include "curve.cuh"

namespace zkmi {

// ---- per-curve pairing parameters --------------------------------------------------------------------------------------------
template <class C> struct PairingCfg;
template <> struct PairingCfg<Bn254Fq> {
    using Fr = Bn254Fr;
    static constexpr uint32_t XI_S = 9, B = 3;
    static constexpr bool D_TWIST = true, BN_END = true;
    static constexpr uint64_t LOOP_HI = 0x1ull, LOOP_LO = 0x9d797039be763ba8ull;      // 6x + 2 = 29793968203157093288
    static constexpr int LOOP_BITS = 65;
};
template <> struct PairingCfg<Bls12381Fq> {
    using Fr = Bls12381Fr;
    static constexpr uint32_t XI_S = 1, B = 4;
    static constexpr bool D_TWIST = false, BN_END = false;
    static constexpr uint64_t LOOP_HI = 0x0ull, LOOP_LO = 0xd201000000010000ull;      // |x|
    static constexpr int LOOP_BITS = 64;
};
template <class C> ZK_HD constexpr bool loop_bit(int i) {
    return i >= 64 ? ((PairingCfg<C>::LOOP_HI >> (i - 64)) & 1) : ((PairingCfg<C>::LOOP_LO >> i) & 1);
}
// lines per G2 point: one per doubling, one per set bit below the top, two Frobenius additions on BN254
template <class C> ZK_HD constexpr int miller_lines() {
    int n = 0;
    for (int i = PairingCfg<C>::LOOP_BITS - 2; i >= 0; i--) n += 1 + (loop_bit<C>(i) ? 1 : 0);
    return n + (PairingCfg<C>::BN_END ? 2 : 0);
}

template <class C> struct Fp6 { Fp2<C> c0, c1, c2; };
template <class C> struct Fp12 { Fp6<C> c0, c1; };
// Constants of one curve (Montgomery form), built on the host: g1[k] = xi^(k(p-1)/6), g2[k] = xi^(k(p^2-1)/6) (in Fq), the twist's b,
// the hard part (p^4 - p^2 + 1)/r of the final exponent as little-endian words.
template <class C> struct PairingConsts {
    Fp2<C> g1[6], g2[6], twist_b;
    Fp<C> b;
    uint32_t hard[48];
    uint32_t hard_bits;
};
// one Miller-loop line, evaluated at P = (px, py) as  a * py  +  b * (-px)  +  c  in the sparse positions of the twist type
template <class C> struct Line { Fp2<C> a, b, c; };
template <class C> struct G2J { Fp2<C> X, Y, Z; };

#define ZK_PAIR_OP __device__ __noinline__

// ---- Fq2 helpers --------------------------------------------------------------------------------------------------------------
template <class C> ZK_DEV Fp2<C> f2_conj(const Fp2<C>& a) { return Fp2<C>{a.c0, fp_neg(a.c1)}; }
template <class C> ZK_DEV Fp2<C> f2_mul_fp(const Fp2<C>& a, const Fp<C>& k) { return Fp2<C>{fp2_base_mul(a.c0, k), fp2_base_mul(a.c1, k)}; }
template <class C> ZK_DEV Fp2<C> f2_mul_xi(const Fp2<C>& a) {
    if constexpr (PairingCfg<C>::XI_S == 1) {
        return Fp2<C>{fp_sub(a.c0, a.c1), fp_add(a.c0, a.c1)};
    } else {
        static_assert(PairingCfg<C>::XI_S == 9, "xi = 1 + u or 9 + u");
        Fp<C> t0 = fp_add(fp_dbl(fp_dbl(fp_dbl(a.c0))), a.c0), t1 = fp_add(fp_dbl(fp_dbl(fp_dbl(a.c1))), a.c1);
        return Fp2<C>{fp_sub(t0, a.c1), fp_add(t1, a.c0)};
    }
}
template <class C> ZK_DEV Fp2<C> f2_zero() { Fp2<C> r; f_set_zero(r); return r; }
template <class C> ZK_DEV Fp2<C> f2_one() { Fp2<C> r; f_set_one(r); return r; }

// ---- Fq6 ----------------------------------------------------------------------------------------------------------------------
template <class C> ZK_DEV Fp6<C> f6_add(const Fp6<C>& a, const Fp6<C>& b) { return Fp6<C>{f_add(a.c0, b.c0), f_add(a.c1, b.c1), f_add(a.c2, b.c2)}; }
template <class C> ZK_DEV Fp6<C> f6_sub(const Fp6<C>& a, const Fp6<C>& b) { return Fp6<C>{f_sub(a.c0, b.c0), f_sub(a.c1, b.c1), f_sub(a.c2, b.c2)}; }
template <class C> ZK_DEV Fp6<C> f6_neg(const Fp6<C>& a) { return Fp6<C>{f_neg(a.c0), f_neg(a.c1), f_neg(a.c2)}; }
template <class C> ZK_DEV Fp6<C> f6_mul_v(const Fp6<C>& a) { return Fp6<C>{f2_mul_xi(a.c2), a.c0, a.c1}; }
template <class C> ZK_DEV Fp6<C> f6_zero() { return Fp6<C>{f2_zero<C>(), f2_zero<C>(), f2_zero<C>()}; }
// Karatsuba over three terms: 6 Fq2 products
template <class C> ZK_PAIR_OP Fp6<C> f6_mul(const Fp6<C>& a, const Fp6<C>& b) {
    Fp2<C> t0 = f_mul(a.c0, b.c0), t1 = f_mul(a.c1, b.c1), t2 = f_mul(a.c2, b.c2);
    Fp6<C> r;
    r.c0 = f_add(t0, f2_mul_xi(f_sub(f_sub(f_mul(f_add(a.c1, a.c2), f_add(b.c1, b.c2)), t1), t2)));
    r.c1 = f_add(f_sub(f_sub(f_mul(f_add(a.c0, a.c1), f_add(b.c0, b.c1)), t0), t1), f2_mul_xi(t2));
    r.c2 = f_add(f_sub(f_sub(f_mul(f_add(a.c0, a.c2), f_add(b.c0, b.c2)), t0), t2), t1);
    return r;
}
// a * (b0 + b1 v): 5 Fq2 products (the sparse factor of a line)
template <class C> ZK_PAIR_OP Fp6<C> f6_mul_01(const Fp6<C>& a, const Fp2<C>& b0, const Fp2<C>& b1) {
    Fp2<C> t0 = f_mul(a.c0, b0), t1 = f_mul(a.c1, b1);
    Fp6<C> r;
    r.c0 = f_add(t0, f2_mul_xi(f_sub(f_mul(f_add(a.c1, a.c2), b1), t1)));
    r.c1 = f_sub(f_sub(f_mul(f_add(a.c0, a.c1), f_add(b0, b1)), t0), t1);
    r.c2 = f_add(f_sub(f_mul(f_add(a.c0, a.c2), b0), t0), t1);
    return r;
}
template <class C> ZK_DEV Fp6<C> f6_mul_1(const Fp6<C>& a, const Fp2<C>& b1) {      // a * (b1 v)
    return Fp6<C>{f2_mul_xi(f_mul(a.c2, b1)), f_mul(a.c0, b1), f_mul(a.c1, b1)};
}
template <class C> ZK_PAIR_OP Fp6<C> f6_inv(const Fp6<C>& a) {
    Fp2<C> A = f_sub(f_sqr(a.c0), f2_mul_xi(f_mul(a.c1, a.c2)));
    Fp2<C> B = f_sub(f2_mul_xi(f_sqr(a.c2)), f_mul(a.c0, a.c1));
    Fp2<C> Cc = f_sub(f_sqr(a.c1), f_mul(a.c0, a.c2));
    Fp2<C> F = f_add(f_mul(a.c0, A), f2_mul_xi(f_add(f_mul(a.c2, B), f_mul(a.c1, Cc))));
    Fp2<C> Fi = f_inv(F);
    return Fp6<C>{f_mul(A, Fi), f_mul(B, Fi), f_mul(Cc, Fi)};
}

// ---- Fq12 ---------------------------------------------------------------------------------------------------------------------
template <class C> ZK_DEV Fp12<C> f12_one() { Fp12<C> r; r.c0 = f6_zero<C>(); r.c1 = f6_zero<C>(); r.c0.c0 = f2_one<C>(); return r; }
template <class C> ZK_DEV Fp12<C> f12_conj(const Fp12<C>& a) { return Fp12<C>{a.c0, f6_neg(a.c1)}; }
template <class C> ZK_PAIR_OP Fp12<C> f12_mul(const Fp12<C>& a, const Fp12<C>& b) {
    Fp6<C> t0 = f6_mul(a.c0, b.c0), t1 = f6_mul(a.c1, b.c1);
    Fp12<C> r;
    r.c1 = f6_sub(f6_sub(f6_mul(f6_add(a.c0, a.c1), f6_add(b.c0, b.c1)), t0), t1);
    r.c0 = f6_add(t0, f6_mul_v(t1));
    return r;
}
// complex squaring: 2 Fq6 products
template <class C> ZK_PAIR_OP Fp12<C> f12_sqr(const Fp12<C>& a) {
    Fp6<C> t = f6_mul(a.c0, a.c1);
    Fp6<C> s = f6_mul(f6_add(a.c0, a.c1), f6_add(a.c0, f6_mul_v(a.c1)));
    Fp12<C> r;
    r.c0 = f6_sub(f6_sub(s, t), f6_mul_v(t));
    r.c1 = f6_add(t, t);
    return r;
}
template <class C> ZK_PAIR_OP Fp12<C> f12_inv(const Fp12<C>& a) {
    Fp6<C> t = f6_inv(f6_sub(f6_mul(a.c0, a.c0), f6_mul_v(f6_mul(a.c1, a.c1))));
    return Fp12<C>{f6_mul(a.c0, t), f6_neg(f6_mul(a.c1, t))};
}
// a^(p^n) for n = 1 (g = K.g1, conjugating the coefficients) or n = 2 (g = K.g2)
template <class C> ZK_PAIR_OP Fp12<C> f12_frob(const Fp12<C>& a, const Fp2<C>* g, bool odd) {
    const Fp2<C>* in[6] = {&a.c0.c0, &a.c1.c0, &a.c0.c1, &a.c1.c1, &a.c0.c2, &a.c1.c2};      // coefficient of w^k
    Fp2<C> o[6];
    for (int k = 0; k < 6; k++) {
        Fp2<C> c = odd ? f2_conj(*in[k]) : *in[k];
        o[k] = k == 0 ? c : f_mul(c, g[k]);
    }
    return Fp12<C>{Fp6<C>{o[0], o[2], o[4]}, Fp6<C>{o[1], o[3], o[5]}};
}
template <class C> ZK_DEV bool f12_is_one(const Fp12<C>& a) {
    const Fp12<C> o = f12_one<C>();
    return f_eq(a.c0.c0, o.c0.c0) && f_is_zero(a.c0.c1) && f_is_zero(a.c0.c2) && f_is_zero(a.c1.c0) && f_is_zero(a.c1.c1) && f_is_zero(a.c1.c2);
}
// f * line: D-type l = a py + (b (-px)) w + c w^3 = (a, 0, 0) + (b', c, 0) w;  M-type l = c + b' w^2 + a py w^3 = (c, b', 0) + (0, a py, 0) w
template <class C> ZK_PAIR_OP Fp12<C> f12_mul_line(const Fp12<C>& f, const Line<C>& l, const Fp<C>& npx, const Fp<C>& py) {
    const Fp2<C> la = f2_mul_fp(l.a, py), lb = f2_mul_fp(l.b, npx);
    Fp12<C> r;
    if constexpr (PairingCfg<C>::D_TWIST) {
        // (f0 + f1 w)(g0 + g1 w), g0 = la (scalar in Fq2), g1 = lb + c v
        Fp6<C> t0 = Fp6<C>{f_mul(f.c0.c0, la), f_mul(f.c0.c1, la), f_mul(f.c0.c2, la)};
        Fp6<C> t1 = f6_mul_01(f.c1, lb, l.c);
        r.c1 = f6_sub(f6_sub(f6_mul_01(f6_add(f.c0, f.c1), f_add(la, lb), l.c), t0), t1);
        r.c0 = f6_add(t0, f6_mul_v(t1));
    } else {
        // g0 = c + lb v, g1 = la v
        Fp6<C> t0 = f6_mul_01(f.c0, l.c, lb);
        Fp6<C> t1 = f6_mul_1(f.c1, la);
        r.c1 = f6_sub(f6_sub(f6_mul_01(f6_add(f.c0, f.c1), l.c, f_add(lb, la)), t0), t1);
        r.c0 = f6_add(t0, f6_mul_v(t1));
    }
    return r;
}

// ---- G2 steps with their lines (Jacobian, a = 0) ------------------------------------------------------------------------------
// T <- 2T. Affine line slope lam = 3x^2/(2y); times k = 2 Y Z^3: a = Z3 Z^2, b = 3 X^2 Z^2, c = 3 X^3 - 2 Y^2.
template <class C> ZK_PAIR_OP void g2_dbl_step(G2J<C>& T, Line<C>& l) {
    Fp2<C> A = f_sqr(T.X), Bq = f_sqr(T.Y), Cq = f_sqr(Bq), Z2 = f_sqr(T.Z);
    Fp2<C> M = f_add(f_dbl(A), A);
    Fp2<C> S = f_dbl(f_dbl(f_mul(T.X, Bq)));
    Fp2<C> Z3 = f_dbl(f_mul(T.Y, T.Z));
    l.a = f_mul(Z3, Z2);
    l.b = f_mul(M, Z2);
    l.c = f_sub(f_mul(M, T.X), f_dbl(Bq));
    Fp2<C> X3 = f_sub(f_sqr(M), f_dbl(S));
    T.Y = f_sub(f_mul(M, f_sub(S, X3)), f_dbl(f_dbl(f_dbl(Cq))));
    T.X = X3;
    T.Z = Z3;
}
// T <- T + Q (Q affine). H = xq Z^2 - X, R = yq Z^3 - Y, slope R/(H Z); times k = H Z = Z3: a = Z3, b = R, c = R xq - yq Z3.
template <class C> ZK_PAIR_OP void g2_add_step(G2J<C>& T, const Affine<Fp2<C>>& Q, Line<C>& l) {
    Fp2<C> Z2 = f_sqr(T.Z);
    Fp2<C> H = f_sub(f_mul(Q.x, Z2), T.X);
    Fp2<C> R = f_sub(f_mul(Q.y, f_mul(Z2, T.Z)), T.Y);
    Fp2<C> Z3 = f_mul(T.Z, H);
    l.a = Z3;
    l.b = R;
    l.c = f_sub(f_mul(R, Q.x), f_mul(Q.y, Z3));
    Fp2<C> HH = f_sqr(H), HHH = f_mul(H, HH), V = f_mul(T.X, HH);
    Fp2<C> X3 = f_sub(f_sub(f_sqr(R), HHH), f_dbl(V));
    T.Y = f_sub(f_mul(R, f_sub(V, X3)), f_mul(T.Y, HHH));
    T.X = X3;
    T.Z = Z3;
}
// BN254 end points: Q1 = pi_p(Q) = (conj(x) g1[2], conj(y) g1[3]), -Q2 = (x g2[2], -y g2[3])
template <class C> ZK_DEV Affine<Fp2<C>> twist_frob1(const Affine<Fp2<C>>& Q, const PairingConsts<C>* K) {
    return Affine<Fp2<C>>{f_mul(f2_conj(Q.x), K->g1[2]), f_mul(f2_conj(Q.y), K->g1[3])};
}
template <class C> ZK_DEV Affine<Fp2<C>> twist_neg_frob2(const Affine<Fp2<C>>& Q, const PairingConsts<C>* K) {
    return Affine<Fp2<C>>{f_mul(Q.x, K->g2[2]), f_neg(f_mul(Q.y, K->g2[3]))};
}

// Lines of a fixed G2 point (miller_lines<C>() entries, loop order): built once per verifying key and read by every lane.
template <class C> ZK_PAIR_OP void g2_line_table(const Affine<Fp2<C>>& Q, Line<C>* out, const PairingConsts<C>* K) {
    G2J<C> T{Q.x, Q.y, f2_one<C>()};
    int li = 0;
    for (int i = PairingCfg<C>::LOOP_BITS - 2; i >= 0; i--) {
        Line<C> l;
        g2_dbl_step(T, l);
        out[li++] = l;
        if (loop_bit<C>(i)) { g2_add_step(T, Q, l); out[li++] = l; }
    }
    if constexpr (PairingCfg<C>::BN_END) {
        Line<C> l;
        g2_add_step(T, twist_frob1(Q, K), l);
        out[li++] = l;
        g2_add_step(T, twist_neg_frob2(Q, K), l);
        out[li++] = l;
    }
}

// Multi-Miller loop: one pair with a variable G2 point Q (walked here) at P = (-npx, py), and up to two pairs with fixed G2 points given
// by their line tables. A pair whose `use` flag is off contributes 1.
template <class C> struct FixedPair {
    const Line<C>* tab;
    Fp<C> npx, py;
    bool use;
};
template <class C> ZK_PAIR_OP Fp12<C> miller_multi(const Affine<Fp2<C>>& Q, const Fp<C>& npx, const Fp<C>& py, bool use_var, const FixedPair<C>& F0,
                                                   const FixedPair<C>& F1, const PairingConsts<C>* K) {
    Fp12<C> f = f12_one<C>();
    G2J<C> T{Q.x, Q.y, f2_one<C>()};
    int li = 0;
    Line<C> l;
    for (int i = PairingCfg<C>::LOOP_BITS - 2; i >= 0; i--) {
        if (i != PairingCfg<C>::LOOP_BITS - 2) f = f12_sqr(f);
        if (use_var) { g2_dbl_step(T, l); f = f12_mul_line(f, l, npx, py); }
        if (F0.use) f = f12_mul_line(f, F0.tab[li], F0.npx, F0.py);
        if (F1.use) f = f12_mul_line(f, F1.tab[li], F1.npx, F1.py);
        li++;
        if (loop_bit<C>(i)) {
            if (use_var) { g2_add_step(T, Q, l); f = f12_mul_line(f, l, npx, py); }
            if (F0.use) f = f12_mul_line(f, F0.tab[li], F0.npx, F0.py);
            if (F1.use) f = f12_mul_line(f, F1.tab[li], F1.npx, F1.py);
            li++;
        }
    }
    if constexpr (PairingCfg<C>::BN_END) {
        for (int e = 0; e < 2; e++) {
            if (use_var) { g2_add_step(T, e == 0 ? twist_frob1(Q, K) : twist_neg_frob2(Q, K), l); f = f12_mul_line(f, l, npx, py); }
            if (F0.use) f = f12_mul_line(f, F0.tab[li], F0.npx, F0.py);
            if (F1.use) f = f12_mul_line(f, F1.tab[li], F1.npx, F1.py);
            li++;
        }
    }
    return f;
}

// f^((p^12 - 1)/r), m = 1. f = 0 (only reachable through degenerate lines) gives 0.
template <class C> ZK_PAIR_OP Fp12<C> final_exp(const Fp12<C>& f, const PairingConsts<C>* K) {
    Fp12<C> t = f12_mul(f12_conj(f), f12_inv(f));            // ^(p^6 - 1)
    t = f12_mul(f12_frob(t, K->g2, false), t);               // ^(p^2 + 1)
    Fp12<C> r = t;
    for (int i = (int)K->hard_bits - 2; i >= 0; i--) {
        r = f12_sqr(r);
        if ((K->hard[i >> 5] >> (i & 31)) & 1) r = f12_mul(r, t);
    }
    return r;
}

// ---- the final exponentiation by a chain of powers of x (used by the aggregated check of kzg_aggregate.cuh only) ------------------
// |x| from the loop scalar: BN254 x = ((6x + 2) - 2)/6 (positive), BLS12-381 x = -|x| with |x| the loop scalar itself.
template <class C> ZK_HD constexpr uint64_t curve_x_abs() {
    if constexpr (PairingCfg<C>::BN_END)
        return (uint64_t)(((((unsigned __int128)PairingCfg<C>::LOOP_HI) << 64 | PairingCfg<C>::LOOP_LO) - 2) / 6);
    else
        return PairingCfg<C>::LOOP_LO;
}
// Squaring in the cyclotomic subgroup (Granger-Scott): a^(p^6 + 1) = 1 is assumed. With Fq4 = Fq2[s]/(s^2 - xi) the element splits into three
// Fq4 pairs (c0.c0, c1.c1), (c1.c0, c0.c2), (c0.c1, c1.c2); each is squared (3 Fq2 squarings) and combined as 3 t -+ 2 a: 9 Fq2 squarings.
template <class C> ZK_DEV void f4_sqr(const Fp2<C>& a, const Fp2<C>& b, Fp2<C>& c0, Fp2<C>& c1) {
    const Fp2<C> t0 = f_sqr(a), t1 = f_sqr(b);
    c0 = f_add(f2_mul_xi(t1), t0);
    c1 = f_sub(f_sub(f_sqr(f_add(a, b)), t0), t1);
}
template <class C> ZK_PAIR_OP Fp12<C> f12_cyclo_sqr(const Fp12<C>& a) {
    Fp2<C> t0, t1, t2, t3, t4, t5;
    f4_sqr(a.c0.c0, a.c1.c1, t0, t1);
    f4_sqr(a.c1.c0, a.c0.c2, t2, t3);
    f4_sqr(a.c0.c1, a.c1.c2, t4, t5);
    const Fp2<C> t5x = f2_mul_xi(t5);
    Fp12<C> r;
    r.c0.c0 = f_add(f_dbl(f_sub(t0, a.c0.c0)), t0);
    r.c1.c1 = f_add(f_dbl(f_add(t1, a.c1.c1)), t1);
    r.c0.c1 = f_add(f_dbl(f_sub(t2, a.c0.c1)), t2);
    r.c1.c2 = f_add(f_dbl(f_add(t3, a.c1.c2)), t3);
    r.c1.c0 = f_add(f_dbl(f_add(t5x, a.c1.c0)), t5x);
    r.c0.c2 = f_add(f_dbl(f_sub(t4, a.c0.c2)), t4);
    return r;
}
// a^|x| for a in the cyclotomic subgroup: MSB-first square-and-multiply over the constant bits of |x|
template <class C> ZK_PAIR_OP Fp12<C> f12_cyclo_pow_x(const Fp12<C>& a) {
    constexpr uint64_t X = curve_x_abs<C>();
    Fp12<C> r = a;
    bool top = false;
    for (int i = 63; i >= 0; i--) {
        const bool bit = (X >> i) & 1;
        if (top) {
            r = f12_cyclo_sqr(r);
            if (bit) r = f12_mul(r, a);
        }
        top = top || bit;
    }
    return r;
}
// final_exp(f)^k for a fixed k coprime to r, so "is one" agrees with final_exp on every f (both give 0 for f = 0):
//   BN254      k = 2x(6x^2 + 3x + 1): the hard part is t^(l0 + l1 p + l2 p^2 + l3 p^3) with l0 = 12x^3 + 12x^2 + 6x + 1, l1 = 12x^3 + 6x^2 + 4x,
//              l2 = 12x^3 + 6x^2 + 6x, l3 = 12x^3 + 6x^2 + 4x - 1 (Fuentes-Castaneda, Knapp, Rodriguez-Henriquez, SAC 2011): three powers of x.
//   BLS12-381  k = 3: the hard part is t^((x - 1)^2 (x + p)(x^2 + p^2 - 1) + 3) (Hayashida, Hayasaka, Teruya 2020); x < 0, so a power of x is
//              the conjugate (the inverse, in the cyclotomic subgroup) of the power of |x|: five powers of |x|.
template <class C> ZK_PAIR_OP Fp12<C> final_exp_chain(const Fp12<C>& f, const PairingConsts<C>* K) {
    Fp12<C> t = f12_mul(f12_conj(f), f12_inv(f));            // ^(p^6 - 1)
    t = f12_mul(f12_frob(t, K->g2, false), t);               // ^(p^2 + 1)
    if constexpr (PairingCfg<C>::BN_END) {
        const Fp12<C> fx = f12_cyclo_pow_x(t), f2x = f12_cyclo_sqr(fx);
        const Fp12<C> f6x = f12_mul(f12_cyclo_sqr(f2x), f2x);
        const Fp12<C> f6x2 = f12_cyclo_pow_x(f6x);
        const Fp12<C> f12x3 = f12_cyclo_pow_x(f12_cyclo_sqr(f6x2));
        const Fp12<C> a = f12_mul(f12_mul(f12x3, f6x2), f6x);                   // t^(12x^3 + 6x^2 + 6x) = t^l2
        const Fp12<C> b = f12_mul(a, f12_conj(f2x));                            // t^l1
        Fp12<C> r = f12_mul(f12_mul(a, f6x2), t);                               // t^l0
        r = f12_mul(r, f12_frob(b, K->g1, true));
        r = f12_mul(r, f12_frob(a, K->g2, false));
        return f12_mul(r, f12_frob(f12_frob(f12_mul(b, f12_conj(t)), K->g2, false), K->g1, true));
    } else {
        const Fp12<C> tc = f12_conj(t);
        const Fp12<C> a = f12_mul(f12_conj(f12_cyclo_pow_x(t)), tc);            // t^(x - 1)
        const Fp12<C> b = f12_mul(f12_conj(f12_cyclo_pow_x(a)), f12_conj(a));   // t^((x - 1)^2)
        const Fp12<C> c = f12_mul(f12_conj(f12_cyclo_pow_x(b)), f12_frob(b, K->g1, true));      // ^(x + p)
        const Fp12<C> cx2 = f12_cyclo_pow_x(f12_cyclo_pow_x(c));                // ^(x^2): two conjugations cancel
        const Fp12<C> d = f12_mul(f12_mul(cx2, f12_frob(c, K->g2, false)), f12_conj(c));        // ^(x^2 + p^2 - 1)
        return f12_mul(d, f12_mul(f12_cyclo_sqr(t), t));                        // * t^3
    }
}

// ---- point input in the reference's object form (fromObject): (x, y, z) standard form, little-endian --------------------------
// z = 0: infinity (returned all-zero, flag set); z = 1: affine; otherwise Jacobian (x/z^2, y/z^3). Values >= p are reduced (the
// Montgomery conversion of a value < R is exact), as F.fromObject reduces.
template <class C> ZK_DEV Fp<C> f_to_mont_any(const Fp<C>& a) { return fp_to_mont(a); }
template <class C> ZK_DEV Fp2<C> f_to_mont_any(const Fp2<C>& a) { return Fp2<C>{fp_to_mont(a.c0), fp_to_mont(a.c1)}; }
template <class F> ZK_DEV bool decode_point(const uint32_t* xyz, Affine<F>& out) {
    constexpr int W = FieldWords<F>::value;
    F x, y, z;
    f_load(x, xyz); f_load(y, xyz + W); f_load(z, xyz + 2 * W);
    x = f_to_mont_any(x); y = f_to_mont_any(y); z = f_to_mont_any(z);
    F one; f_set_one(one);
    if (f_is_zero(z)) { f_set_zero(out.x); f_set_zero(out.y); return true; }
    if (f_eq(z, one)) { out.x = x; out.y = y; return false; }
    F zi = f_inv(z), zi2 = f_sqr(zi);
    out.x = f_mul(x, zi2);
    out.y = f_mul(y, f_mul(zi2, zi));
    return false;
}
template <class C> ZK_DEV bool on_curve(const Affine<Fp<C>>& P, const PairingConsts<C>* K) {
    return fp_eq(fp_sqr(P.y), fp_add(fp_mul(fp_sqr(P.x), P.x), K->b));
}
template <class C> ZK_DEV bool on_curve(const Affine<Fp2<C>>& P, const PairingConsts<C>* K) {
    return f_eq(f_sqr(P.y), f_add(f_mul(f_sqr(P.x), P.x), K->twist_b));
}

// ---- Groth16 verification of one proof (src/groth16_verify.js:26-87) ----------------------------------------------------------
template <class C> struct VkView {
    const Fp<C>* ic;              // n_ic affine Montgomery points (x, y); infinity all-zero
    uint32_t n_ic;
    const Line<C>* tab_gamma;     // miller_lines<C>() each
    const Line<C>* tab_delta;
    uint32_t gamma_inf, delta_inf;
    const Fp12<C>* mab;           // Miller value of (alpha_1, beta_2); one when either is infinity
};
enum { G16V_VALID = 1, G16V_INVALID = 0, G16V_BAD_PUBLIC = -1, G16V_BAD_POINT = -2 };

// public signal j: 8 little-endian words, standard form; < r
template <class C> ZK_DEV bool public_below_r(const uint32_t* s) {
    using Fr = typename PairingCfg<C>::Fr;
    unsigned bw = 0;
    for (int i = 0; i < 8; i++) (void)__builtin_subc(s[i], Fr::p(i), bw, &bw);
    return bw != 0;
}
// What a proof that passes the input checks hands to the aggregated check (groth16_aggregate.cuh): its three points and vk_x, affine, Montgomery;
// *_inf set for the point at infinity (the coordinates are then all-zero).
template <class C> struct G16Front {
    Affine<Fp<C>> A, Cp;
    Affine<Fp2<C>> B;
    Fp<C> vx, vy;
    bool a_inf, b_inf, c_inf, x_inf;
};
// proof record: pi_a (3 Fq), pi_b (3 Fq2), pi_c (3 Fq), standard form; publics: n_signals x 8 words.
// With AGG the check stops before the Miller loop and hands over its front half instead (the code is then G16V_VALID for "the input checks
// passed"). Without it (the default: k_g16_verify) the function is what it was.
template <class C, bool AGG = false>
ZK_DEV int groth16_verify_one(const uint32_t* rec, const uint32_t* pubs, uint32_t n_signals, const VkView<C>& vk, const PairingConsts<C>* K,
                              G16Front<C>* front = nullptr) {
    constexpr int N = C::N;
    for (uint32_t j = 0; j < n_signals; j++)
        if (!public_below_r<C>(pubs + 8 * j)) return G16V_BAD_PUBLIC;
    Affine<Fp<C>> A, Cp;
    Affine<Fp2<C>> B;
    const bool a_inf = decode_point(rec, A);
    const bool b_inf = decode_point(rec + 3 * N, B);
    const bool c_inf = decode_point(rec + 9 * N, Cp);
    if (!(a_inf || on_curve(A, K)) || !(b_inf || on_curve(B, K)) || !(c_inf || on_curve(Cp, K))) return G16V_BAD_POINT;
    // vk_x = IC0 + sum_j pub_j IC_{j+1}: interleaved double-and-add over the 256 bits of every public
    XYZZ<Fp<C>> acc;
    pt_set_inf(acc);
    for (int bit = n_signals ? 255 : -1; bit >= 0; bit--) {
        acc = pt_dbl(acc);
        for (uint32_t j = 0; j < n_signals; j++)
            if ((pubs[8 * j + (bit >> 5)] >> (bit & 31)) & 1) pt_madd(acc, Affine<Fp<C>>{vk.ic[2 * (j + 1)], vk.ic[2 * (j + 1) + 1]});
    }
    pt_madd(acc, Affine<Fp<C>>{vk.ic[0], vk.ic[1]});
    const bool x_inf = pt_is_inf(acc);
    Fp<C> vx = fp_zero<C>(), vy = fp_zero<C>();
    if (!x_inf) {
        const Fp<C> i = fp_inv(fp_mul(acc.ZZ, acc.ZZZ));
        vx = fp_mul(acc.X, fp_mul(i, acc.ZZZ));
        vy = fp_mul(acc.Y, fp_mul(i, acc.ZZ));
    }
    if constexpr (AGG) {
        *front = G16Front<C>{A, Cp, B, vx, vy, a_inf, b_inf, c_inf, x_inf};
        return G16V_VALID;
    } else {
        // e(-A, B) e(vk_x, gamma) e(C, delta) e(alpha, beta) == 1; the pairs are passed as (-px, py): -A = (A.x, -A.y)
        const FixedPair<C> g{vk.tab_gamma, fp_neg(vx), vy, !x_inf && !vk.gamma_inf};
        const FixedPair<C> d{vk.tab_delta, fp_neg(Cp.x), Cp.y, !c_inf && !vk.delta_inf};
        Fp12<C> f = miller_multi(B, fp_neg(A.x), fp_neg(A.y), !a_inf && !b_inf, g, d, K);
        f = f12_mul(f, *vk.mab);
        return f12_is_one(final_exp(f, K)) ? G16V_VALID : G16V_INVALID;
    }
}

// Fq12 (tower) -> the oracle's w-basis, 12 Fq coefficients in standard form: c_k = a + b u -> (a - s b) w^k + b w^(k+6)
template <class C> ZK_DEV void f12_to_wbasis(const Fp12<C>& a, Fp<C>* out) {
    const Fp2<C>* in[6] = {&a.c0.c0, &a.c1.c0, &a.c0.c1, &a.c1.c1, &a.c0.c2, &a.c1.c2};
    Fp<C> s = fp_zero<C>();
    s.l[0] = PairingCfg<C>::XI_S;
    s = fp_to_mont(s);
    for (int k = 0; k < 6; k++) {
        out[k] = fp_from_mont(fp_sub(in[k]->c0, fp_mul(s, in[k]->c1)));
        out[k + 6] = fp_from_mont(in[k]->c1);
    }
}

// ---- per verifying key: points to Montgomery form, line tables of beta, gamma, delta, M(alpha, beta) (one lane) ------------------
// ic_out: n_ic affine points (x, y), infinity all-zero; returns bit 0: gamma at infinity, bit 1: delta at infinity.
template <class C> ZK_PAIR_OP uint32_t vk_prepare(const uint32_t* alpha_xyz, const uint32_t* beta_xyz, const uint32_t* gamma_xyz, const uint32_t* delta_xyz,
                                                  const uint32_t* ic_xyz, uint32_t n_ic, const PairingConsts<C>* K, Fp<C>* ic_out, Line<C>* tab_beta,
                                                  Line<C>* tab_gamma, Line<C>* tab_delta, Fp12<C>* mab) {
    for (uint32_t i = 0; i < n_ic; i++) {
        Affine<Fp<C>> P;
        decode_point(ic_xyz + 3 * C::N * i, P);
        ic_out[2 * i] = P.x;
        ic_out[2 * i + 1] = P.y;
    }
    Affine<Fp<C>> al;
    Affine<Fp2<C>> be, ga, de;
    const bool al_inf = decode_point(alpha_xyz, al), be_inf = decode_point(beta_xyz, be);
    const bool ga_inf = decode_point(gamma_xyz, ga), de_inf = decode_point(delta_xyz, de);
    if (!be_inf) g2_line_table(be, tab_beta, K);
    if (!ga_inf) g2_line_table(ga, tab_gamma, K);
    if (!de_inf) g2_line_table(de, tab_delta, K);
    const FixedPair<C> ab{tab_beta, fp_neg(al.x), al.y, !al_inf && !be_inf};
    const FixedPair<C> none{tab_beta, al.x, al.y, false};
    *mab = miller_multi(be, al.x, al.y, false, ab, none, K);
    return (ga_inf ? 1u : 0u) | (de_inf ? 2u : 0u);
}

// reduced pairing e(P, Q) of one pair in the oracle's w-basis (standard form); either point at infinity gives 1
template <class C> ZK_PAIR_OP void pairing_one(const uint32_t* g1_xyz, const uint32_t* g2_xyz, const PairingConsts<C>* K, Fp<C>* out12) {
    Affine<Fp<C>> P;
    Affine<Fp2<C>> Q;
    const bool p_inf = decode_point(g1_xyz, P), q_inf = decode_point(g2_xyz, Q);
    const bool inf = p_inf || q_inf;
    const FixedPair<C> none{nullptr, P.x, P.y, false};
    Fp12<C> f = inf ? f12_one<C>() : final_exp(miller_multi(Q, fp_neg(P.x), P.y, true, none, none, K), K);
    f12_to_wbasis(f, out12);
}

}  // namespace zkmi
