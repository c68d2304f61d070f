// snarkjs_amd/csrc/groth16_setup.cuh — device kernels of the Groth16 setup (zkey new) for gfx950.
//
// Replaces the task lists the reference sends straight to its workers in composeAndWritePointsThread (src/zkey_new.js:383-501:
// g1m_/g2m_multiexpAffine, _timesScalarAffine, _zero, _batchToAffine per signal) and hashHPointsThread (:544-577: g1m_subAffine,
// _batchToAffine, _batchLEMtoU). Every output point of sections 3 and 5-8 is a short linear combination
//     P_s = sum_j coef_j * Base[table_j][constraint_j]
// over one column of the constraint matrices. The host (groth16_setup.hip) cuts every column into SEGMENTS of at most SETUP_SEG terms,
// recodes every coefficient as sign and magnitude (c > r/2 -> r - c with the base negated) and sorts the segments by (top bit, length), so
// that the lanes of a wavefront run the same trip count.
//   k_setup_eval    one lane per segment: one double-and-add shared by the terms of the segment, from the segment's top bit down. A
//                   segment of +-1 terms (the common case) is one pass of mixed additions, a 2^k term costs k doublings and one addition.
//   k_setup_fold    one lane per output: the sum of a run of partial sums (levels of at most SETUP_FOLD until one point per column is left;
//                   a column without terms comes out as infinity = the reference's all-zero bytes).
//   k_setup_affine  XYZZ -> affine Montgomery, SETUP_INV points per lane behind ONE inversion (Montgomery's trick on ZZZ).
//   k_setup_hdiff   tauG1[i + domain] - tauG1[i], the H points that enter the circuit hash.
// The accumulator of a lane lives in LDS (LdsAcc, curve.cuh): an Fq2 XYZZ point plus the operands of an addition do not fit the
// register file. Integer arithmetic only, no atomics: group addition is exact on the affine result, so the order of the partial sums
// cannot change a byte.
#pragma once
#include "curve.cuh"

namespace zkmi {

constexpr int SETUP_SEG = 32;      // terms per segment
constexpr int SETUP_FOLD = 32;     // partial sums per lane and fold level
constexpr int SETUP_T = 128;       // lanes per block: 4 coordinates x 24 words x 128 lanes = 48 KiB of LDS for BLS12-381 G2
constexpr int SETUP_INV = 4;       // points per inversion

template <class F, int T> ZK_DEV void setup_store_acc(uint32_t* dst, const LdsAcc<F, T>& A, bool inf) {
    constexpr int FW = FieldWords<F>::value;
    if (inf) {
#pragma unroll
        for (int k = 0; k < 4 * FW; k++) dst[k] = 0u;
        return;
    }
#pragma unroll
    for (int c = 0; c < 4; c++) { F v; A.get(c, v); f_store(dst + c * FW, v); }
}

// terms: x = base index | sign << 31, y = 0 for magnitude 1, else 1 + index into mags (8 words each, plain little-endian integers below r/2)
// segs:  x = first term, y = number of terms, z = top bit of the widest magnitude, w = slot of the partial sum
template <class F, int T> __global__ void __launch_bounds__(T)
k_setup_eval(const uint32_t* __restrict__ bases, const uint2* __restrict__ terms, const uint4* __restrict__ segs, const uint32_t* __restrict__ mags,
             uint32_t* __restrict__ part, uint32_t n_seg) {
    constexpr int FW = FieldWords<F>::value;
    __shared__ uint32_t lds[4 * FW * T];
    const uint32_t i = blockIdx.x * T + threadIdx.x;
    if (i >= n_seg) return;
    const uint4 sg = segs[i];
    const LdsAcc<F, T> A{lds + threadIdx.x};
    bool inf = true;
    for (int bit = (int)sg.z; bit >= 0; bit--) {
        if (!inf && bit != (int)sg.z) pt_dbl_lds(A);
        for (uint32_t j = 0; j < sg.y; j++) {
            const uint2 t = terms[sg.x + j];
            const bool set = t.y ? ((mags[(size_t)(t.y - 1u) * 8 + (bit >> 5)] >> (bit & 31)) & 1u) != 0u : bit == 0;
            if (!set) continue;
            Affine<F> q;
            pt_load(q, bases + (size_t)(t.x & 0x7fffffffu) * 2 * FW);
            if (pt_is_inf(q)) continue;
            if (t.x >> 31) q.y = f_neg(q.y);
            pt_madd_lds(A, inf, q);
        }
    }
    setup_store_acc(part + (size_t)sg.w * 4 * FW, A, inf);
}

// out[i] = sum of in[off[i] .. off[i + 1])
template <class F, int T> __global__ void __launch_bounds__(T)
k_setup_fold(const uint32_t* __restrict__ in, const uint32_t* __restrict__ off, uint32_t* __restrict__ out, uint32_t n_out) {
    constexpr int FW = FieldWords<F>::value;
    __shared__ uint32_t lds[4 * FW * T];
    const uint32_t i = blockIdx.x * T + threadIdx.x;
    if (i >= n_out) return;
    const LdsAcc<F, T> A{lds + threadIdx.x};
    bool inf = true;
    const uint32_t e = off[i + 1];
    for (uint32_t k = off[i]; k < e; k++) {
        const uint32_t* p = in + (size_t)k * 4 * FW;
        pt_add_lds(A, inf, [&](int c, F& v) { f_load(v, p + c * FW); });
    }
    setup_store_acc(out + (size_t)i * 4 * FW, A, inf);
}

// XYZZ -> affine (x = X / ZZ, y = Y / ZZZ with 1 / ZZ = (ZZ / ZZZ)^2); infinity -> all zero
template <class F> __global__ void __launch_bounds__(256)
k_setup_affine(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    constexpr int FW = FieldWords<F>::value, K = SETUP_INV;
    const uint32_t i0 = (blockIdx.x * 256 + threadIdx.x) * K;
    if (i0 >= n) return;
    F pre[K], run;
    f_set_one(run);
#pragma unroll
    for (int k = 0; k < K; k++) {
        pre[k] = run;
        if (i0 + k < n) {
            F z;
            f_load(z, in + (size_t)(i0 + k) * 4 * FW + 3 * FW);
            if (!f_is_zero(z)) run = f_mul(run, z);
        }
    }
    F inv = f_inv(run);
#pragma unroll
    for (int k = K - 1; k >= 0; k--) {
        if (i0 + k < n) {
            const uint32_t* src = in + (size_t)(i0 + k) * 4 * FW;
            uint32_t* dst = out + (size_t)(i0 + k) * 2 * FW;
            F z, x, y;
            f_load(z, src + 3 * FW);
            const bool inf = f_is_zero(z);
            if (!inf) {
                const F i3 = f_mul(inv, pre[k]);
                inv = f_mul(inv, z);
                F t;
                f_load(t, src + 2 * FW);
                const F i2 = f_sqr(f_mul(t, i3));
                f_load(t, src);
                x = f_mul(t, i2);
                f_load(t, src + FW);
                y = f_mul(t, i3);
            } else { f_set_zero(x); f_set_zero(y); }
            f_store(dst, x);
            f_store(dst + FW, y);
        }
    }
}

// out[i] = tau[i + domain] - tau[i] (affine in, XYZZ out)
template <class F> __global__ void __launch_bounds__(256)
k_setup_hdiff(const uint32_t* __restrict__ tau, uint32_t* __restrict__ out, uint32_t n, uint32_t domain) {
    constexpr int FW = FieldWords<F>::value;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Affine<F> a, b;
    pt_load(a, tau + (size_t)(i + domain) * 2 * FW);
    pt_load(b, tau + (size_t)i * 2 * FW);
    XYZZ<F> acc;
    if (pt_is_inf(a)) pt_set_inf(acc);
    else { acc.X = a.x; acc.Y = a.y; f_set_one(acc.ZZ); f_set_one(acc.ZZZ); }
    b.y = f_neg(b.y);
    pt_madd(acc, b);
    pt_store(out + (size_t)i * 4 * FW, acc);
}

}  // namespace zkmi
