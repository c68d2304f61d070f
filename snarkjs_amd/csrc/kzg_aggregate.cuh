// snarkjs_amd/csrc/kzg_aggregate.cuh — the aggregated ("are all of these valid?") check that PLONK and FFLONK share, gfx950.
//
// Both protocols end in e(-P_i, T0) e(Q_i, T1) == 1 with T0, T1 fixed per key (PLONK: P = A1, Q = B1, T0 = X_2, T1 = [1]_2; FFLONK: P = A1,
// Q = W2, T0 = [1]_2, T1 = X_2). For a batch under one key and a 32-byte seed:
//     r_i = the first 16 bytes, little-endian, of Keccak-256(seed | LE64(i)), bit 127 set          (agg_challenge)
//     S_P = sum r_i P_i,  S_Q = sum r_i Q_i  over the lanes whose input checks pass                (agg_scale, agg_block_sum, agg_fold)
//     ok  = every lane's code is 1  and  e(-S_P, T0) e(S_Q, T1) == 1                               (agg_tail)
// One Miller loop and one final exponentiation per batch instead of one per proof. The tail runs on one lane, so it uses the chain final
// exponentiation (pairing.cuh final_exp_chain), not the plain hard part.
//
// A lane whose input checks fail reports its code and contributes the point at infinity. The additions are complete (curve.cuh pt_add: infinity,
// equal and opposite operands). On BLS12-381 the tail multiplies both sums by the G1 cofactor h = (x - 1)^2 / 3 first: a proof point on the curve
// outside G1 then enters through its G1 component only. The sums reported to a trace are the sums before that multiplication.
//
// Like kzg_verify.cuh this is __device__ code that also compiles for the host (tools/aggregate_verify_hosttest.hip, __device__ defined away).
#pragma once
#include "kzg_verify.cuh"

namespace zkmi {

enum { AGG_ENTERED = 1 };                      // a lane's code when its pair entered the sums (the per-proof codes <= 0 keep their meaning)

// r_i as two 64-bit halves. The message is five whole lanes; the digest's first sixteen bytes are the first two lanes of the squeezed state.
ZK_DEV void agg_challenge(const uint64_t* seed4, uint64_t i, uint64_t& lo, uint64_t& hi) {
    Keccak256 k;
    keccak_init(k);
    for (int j = 0; j < 4; j++) keccak_lane(k, seed4[j]);
    keccak_lane(k, i);
    uint32_t d[8];
    keccak_finish(k, d);
    lo = k.st[0];
    hi = k.st[1] | 0x8000000000000000ull;
}

// r * P for a 128-bit r with its top bit set: 127 doublings, one mixed addition per further set bit. P at infinity (fin off) gives infinity.
template <class C> ZK_DEV XYZZ<Fp<C>> agg_scale(const Fp<C>& x, const Fp<C>& y, bool fin, uint64_t lo, uint64_t hi) {
    XYZZ<Fp<C>> acc;
    pt_set_inf(acc);
    if (!fin) return acc;
    const Affine<Fp<C>> P{x, y};
    pt_madd(acc, P);
    for (int bit = 126; bit >= 0; bit--) {
        acc = pt_dbl(acc);
        if (((bit >= 64 ? hi >> (bit - 64) : lo >> bit) & 1) != 0) pt_madd(acc, P);
    }
    return acc;
}

// the G1 cofactor as two 64-bit halves: 1 on BN254, (|x| + 1)^2 / 3 on BLS12-381 (x < 0), from the loop scalar
template <class C> ZK_HD constexpr unsigned __int128 g1_cofactor() {
    if constexpr (PairingCfg<C>::BN_END) return 1;
    else return ((unsigned __int128)(curve_x_abs<C>() + 1) * (curve_x_abs<C>() + 1)) / 3;
}
template <class C> ZK_DEV XYZZ<Fp<C>> agg_clear_cofactor(const XYZZ<Fp<C>>& p) {
    constexpr unsigned __int128 H = g1_cofactor<C>();
    if constexpr (H == 1) return p;
    XYZZ<Fp<C>> acc;
    pt_set_inf(acc);
    for (int bit = 127; bit >= 0; bit--) {
        acc = pt_dbl(acc);
        if ((uint64_t)(H >> bit) & 1) acc = pt_add(acc, p);
    }
    return acc;
}

// One pair of partial sums.
template <class C> struct AggPair { XYZZ<Fp<C>> p, q; };

// Sum of the T pairs of a block (T a power of two, one pair per thread) by a tree in sh (T entries): the result is in sh[0] after the call.
// Every thread of the block must call it. On the host (T = 1) it is the identity.
template <class C, int T> ZK_DEV void agg_block_sum(AggPair<C>* sh, unsigned t, const AggPair<C>& mine) {
    sh[t] = mine;
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
    for (unsigned s = T / 2; s > 0; s >>= 1) {
        if (t < s) {
            sh[t].p = pt_add(sh[t].p, sh[t + s].p);
            sh[t].q = pt_add(sh[t].q, sh[t + s].q);
        }
        __syncthreads();
    }
#endif
}

// what the tail reports: the pairing verdict and the two sums, affine, standard form (x | y each; infinity all-zero)
template <class C> struct AggResult {
    uint32_t pair_ok;
    uint32_t sp[2 * C::N], sq[2 * C::N];
};

// The tail: S_P, S_Q (XYZZ) -> the report. tab0 / tab1 are the line tables of T0 / T1; use0 / use1 are off where that G2 point is the point at
// infinity (its pair then contributes 1, as a pair with a sum at infinity does).
template <class C> ZK_PAIR_OP void agg_tail(const AggPair<C>& S, const Line<C>* tab0, const Line<C>* tab1, bool use0, bool use1, const PairingConsts<C>* K, AggResult<C>* out) {
    constexpr int N = C::N;
    Fp<C> x, y;
    (void)xyzz_to_affine(S.p, x, y);
    Fp<C> sx = fp_from_mont(x), sy = fp_from_mont(y);
    for (int i = 0; i < N; i++) { out->sp[i] = sx.l[i]; out->sp[N + i] = sy.l[i]; }
    (void)xyzz_to_affine(S.q, x, y);
    sx = fp_from_mont(x); sy = fp_from_mont(y);
    for (int i = 0; i < N; i++) { out->sq[i] = sx.l[i]; out->sq[N + i] = sy.l[i]; }
    Fp<C> px, py, qx, qy;
    const bool p_fin = xyzz_to_affine(agg_clear_cofactor<C>(S.p), px, py);
    const bool q_fin = xyzz_to_affine(agg_clear_cofactor<C>(S.q), qx, qy);
    // e(-S_P, T0) e(S_Q, T1) == 1; pairs are passed as (-px, py)
    const FixedPair<C> f0{tab0, fp_neg(px), fp_neg(py), p_fin && use0};
    const FixedPair<C> f1{tab1, fp_neg(qx), qy, q_fin && use1};
    Affine<Fp2<C>> none;
    f_set_zero(none.x);
    f_set_zero(none.y);
    const Fp12<C> f = miller_multi(none, px, py, false, f0, f1, K);
    out->pair_ok = f12_is_one(final_exp_chain(f, K)) ? 1u : 0u;
}

}  // namespace zkmi
