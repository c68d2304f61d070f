// snarkjs_amd/csrc/ptau_lagrange.cuh — the Lagrange sections 12 - 15 of a prepared .ptau for gfx950 (src/powersoftau_preparephase2.js): for
// p = first .. top the inverse group FFT of the first 2^p points of ONE source section, all powers in one pass of top + 2 launches.
//
// The work array IS the Lagrange section, as XYZZ points on the 32-bit limbs of curve.cuh (both groups): block p holds 2^p points at point offset
// 2^p - 2^first. Every block runs the radix-2 decimation-in-time butterflies of gfft.cuh over its own bit-reversed load, and the twiddle of the butterfly at
// stage st, index j is w_{2^st}^-j whatever the block's size. So one launch per stage serves all blocks p >= st, with the lanes laid out TWIDDLE-MAJOR: lane
// t = j * 2^(top-st+1) + m' holds twiddle j; slot m' = 0 is idle, slot m' > 0 is group g = m' - 2^(p-st) of block p = st + ilog2(m'). From 64 slots per twiddle
// up a wave holds one twiddle, recodes one scalar and walks one digit stream: the data-dependent branch of pt_mul_naf is taken by all lanes or by none.
//   k_ptau_lag_load    lane -> (p, i): block p receives source point i at place bitrev_p(i); with zero_last the last point of the top block is infinity
//   k_ptau_lag_stage   one DIT stage over all blocks p >= max(st, first): (a, b) -> (a + w b, a - w b) with the complete addition pt_add
//   k_ptau_lag_store   lane t - 2^first -> point t - 1 of the section: times 2^-p (p = ilog2(t), shared by a wave from p = 6 up), to affine Montgomery
// The three lane maps are __host__ __device__: tools/ptau_lagrange_hosttest.hip enumerates them on the CPU.
#pragma once
#include "gfft.cuh"

namespace zkmi {

constexpr uint32_t PTAU_LAG_MAX_TOP = 28;        // 2^29 - 1 points of work at most: every point offset fits 32 bits

ZK_HD uint32_t lag_ilog2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }                  // v > 0
ZK_HD uint32_t lag_bitrev(uint32_t i, uint32_t bits) {
    uint32_t r = 0;
    for (uint32_t b = 0; b < bits; b++) r |= ((i >> b) & 1u) << (bits - 1 - b);
    return r;
}
// point offset of block p in a work array / an output that holds the blocks first .. top back to back
ZK_HD uint32_t lag_block_base(uint32_t p, uint32_t first) { return (1u << p) - (1u << first); }
ZK_HD uint32_t lag_points(uint32_t first, uint32_t top) { return (2u << top) - (1u << first); }

// load and store: lane tid < lag_points(first, top) is point tid of the output; t = tid + 2^first numbers the points of a whole section from 1
struct LagPoint { uint32_t p, i; };
ZK_HD LagPoint lag_point_of(uint32_t tid, uint32_t first) {
    const uint32_t t = tid + (1u << first), p = lag_ilog2(t);
    return LagPoint{p, t - (1u << p)};
}
// where the load puts source point i of block p
ZK_HD uint32_t lag_load_dst(const LagPoint& q, uint32_t first) { return lag_block_base(q.p, first) + lag_bitrev(q.i, q.p); }

// one butterfly of stage st (1 .. top); lanes t < 2^top. e is the exponent of the twiddle in the inverse power tables of the 2^top transform
struct LagButterfly { bool idle; uint32_t p, j, lo, hi; uint64_t e; };
ZK_HD LagButterfly lag_stage_lane(uint32_t t, uint32_t st, uint32_t first, uint32_t top) {
    const uint32_t ls = top - st + 1, m = t & ((1u << ls) - 1u), j = t >> ls;
    LagButterfly r{true, 0, j, 0, 0, 0};
    if (!m) return r;
    const uint32_t q = lag_ilog2(m), p = st + q;
    if (p < first) return r;
    const uint32_t g = m - (1u << q);
    r.idle = false; r.p = p;
    r.lo = lag_block_base(p, first) + (g << st) + j;
    r.hi = r.lo + (1u << (st - 1));
    r.e = (uint64_t)j << (top - st);
    return r;
}

#if defined(__HIPCC__)
template <class F> __global__ void __launch_bounds__(256)
k_ptau_lag_load(const uint32_t* __restrict__ in, uint32_t* __restrict__ work, uint32_t first, uint32_t top, int zero_last) {
    constexpr int FW = FieldWords<F>::value;
    const uint32_t tid = blockIdx.x * 256 + threadIdx.x;
    if (tid >= lag_points(first, top)) return;
    const LagPoint q = lag_point_of(tid, first);
    XYZZ<F> pt;
    if (zero_last && q.p == top && q.i == (1u << top) - 1u) pt_set_inf(pt);
    else {
        Affine<F> a; pt_load(a, in + (size_t)q.i * 2 * FW);
        pt = pt_from_affine(a);
    }
    pt_store(work + (size_t)lag_load_dst(q, first) * 4 * FW, pt);
}

template <class F, class FrC> __global__ void __launch_bounds__(256)
k_ptau_lag_stage(uint32_t* __restrict__ work, uint32_t st, uint32_t first, uint32_t top, GfftTw tw) {
    constexpr int PW = 4 * FieldWords<F>::value;
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= (1u << top)) return;
    const LagButterfly bf = lag_stage_lane(t, st, first, top);
    if (bf.idle) return;
    XYZZ<F> A, B;
    pt_load(A, work + (size_t)bf.lo * PW); pt_load(B, work + (size_t)bf.hi * PW);
    if (bf.j) {
        const Fp<FrC> lo_t = fp_load<FrC>(tw.T_lo + (size_t)(bf.e & ((1ull << tw.log_lb) - 1)) * 8), hi_t = fp_load<FrC>(tw.T_hi + (size_t)(bf.e >> tw.log_lb) * 8);
        uint32_t k[8];
        fr_to_scalar<FrC>(k, fp_mul(lo_t, hi_t));
        B = pt_mul_naf<F>(B, k);
    }
    XYZZ<F> nB = B;
    nB.Y = f_neg(nB.Y);
    pt_store(work + (size_t)bf.lo * PW, pt_add(A, B));
    pt_store(work + (size_t)bf.hi * PW, pt_add(A, nB));
}

// inv2: 2^-p for p = 0 .. top as plain 256-bit scalars (8 words each, normal form)
template <class F> __global__ void __launch_bounds__(256)
k_ptau_lag_store(const uint32_t* __restrict__ work, uint32_t* __restrict__ out, uint32_t first, uint32_t top, const uint32_t* __restrict__ inv2) {
    constexpr int FW = FieldWords<F>::value;
    const uint32_t tid = blockIdx.x * 256 + threadIdx.x;
    if (tid >= lag_points(first, top)) return;
    const uint32_t p = lag_point_of(tid, first).p;
    XYZZ<F> pt; pt_load(pt, work + (size_t)tid * 4 * FW);
    if (p) {
        uint32_t k[8];
#pragma unroll
        for (int i = 0; i < 8; i++) k[i] = inv2[p * 8 + i];
        pt = pt_mul_naf<F>(pt, k);
    }
    const Affine<F> a = pt_to_affine(pt);
    f_store(out + (size_t)tid * 2 * FW, a.x); f_store(out + (size_t)tid * 2 * FW + FW, a.y);
}
#endif

}  // namespace zkmi
