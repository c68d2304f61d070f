// snarkjs_amd/csrc/r1cs_check.cuh — kernels of the witness check (snarkjs.wtns.check, reference src/wtns_check.js) and the routines one lane of them runs.
//
// Constraint i holds iff evalA * evalB == evalC in Fr, each evaluation the sum of coef * w[signal] over the DISTINCT signals of the combination with the
// LAST coefficient the file gives for a signal (the reference's reader writes lc[idx] = val). Coefficients and witness values are any 256-bit value, taken
// mod r (Fr.fromRprLE).
//
// Layout, once per r1cs: the sliced ELL with split rows of abc_layout.cuh over rows = 3 * constraint + matrix; a term's value is kept times R^2 as zkey
// section 4 keeps it, so its Montgomery product with a witness value in normal form is (coef * w) R. A repeated signal: every term that a LATER term of the
// same combination repeats gets coefficient 0, which is exact (0 * w adds nothing) and leaves the walk untouched.
//
// The lane routines (r1cs_reduce256, r1cs_mul, r1cs_coef, r1cs_holds) are __host__ __device__: on the device the product is fp_mul of field.cuh, on the host
// (tools/r1cs_check_hosttest.hip) a plain operand-scanning Montgomery product stands in for it; everything around the product is the same code.
#pragma once
#include "abc_layout.cuh"
#include "field.cuh"

namespace zkmi {

// ---- lane routines --------------------------------------------------------------------------------------------------------------------------
// v < 2^256 -> v mod r. 2^256 < 6 r for both scalar fields (5 r < 2^256 on BN254, 2 r < 2^256 on BLS12-381): five conditional subtractions.
template <class C> ZK_HD void r1cs_reduce256(Fp<C>& v) {
    static_assert(C::N == 8 && C::p(7) > 0x2aaaaaaau, "r1cs_reduce256 needs 6 r > 2^256");
#pragma unroll
    for (int round = 0; round < 5; round++) {
        uint32_t d[8];
        uint32_t bw = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint64_t x = (uint64_t)v.l[i] - C::p(i) - bw;
            d[i] = (uint32_t)x;
            bw = (uint32_t)(x >> 32) & 1u;
        }
#pragma unroll
        for (int i = 0; i < 8; i++) v.l[i] = bw ? v.l[i] : d[i];
    }
}
// Montgomery product a b / R mod r, fully reduced
template <class C> ZK_HD Fp<C> r1cs_mul(const Fp<C>& a, const Fp<C>& b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return fp_mul(a, b);
#else
    constexpr int N = C::N;
    uint32_t t[N + 2] = {};
    for (int i = 0; i < N; i++) {
        uint64_t c = 0;
        for (int j = 0; j < N; j++) { const uint64_t x = (uint64_t)a.l[j] * b.l[i] + t[j] + c; t[j] = (uint32_t)x; c = x >> 32; }
        uint64_t x = (uint64_t)t[N] + c;
        t[N] = (uint32_t)x; t[N + 1] = (uint32_t)(x >> 32);
        const uint32_t m = t[0] * C::NP;
        c = ((uint64_t)m * C::p(0) + t[0]) >> 32;
        for (int j = 1; j < N; j++) { const uint64_t y = (uint64_t)m * C::p(j) + t[j] + c; t[j - 1] = (uint32_t)y; c = y >> 32; }
        x = (uint64_t)t[N] + c;
        t[N - 1] = (uint32_t)x; t[N] = t[N + 1] + (uint32_t)(x >> 32);
    }
    uint32_t d[N];
    uint32_t bw = 0;
    for (int i = 0; i < N; i++) { const uint64_t x = (uint64_t)t[i] - C::p(i) - bw; d[i] = (uint32_t)x; bw = (uint32_t)(x >> 32) & 1u; }
    Fp<C> r;
    for (int i = 0; i < N; i++) r.l[i] = (t[N] || !bw) ? d[i] : t[i];
    return r;
#endif
}
// a coefficient as the layout keeps it: (c mod r) R^2 mod r
template <class C> ZK_HD Fp<C> r1cs_coef(Fp<C> c) {
    Fp<C> r2;
#pragma unroll
    for (int i = 0; i < C::N; i++) r2.l[i] = C::r2(i);
    r1cs_reduce256<C>(c);
    return r1cs_mul<C>(r1cs_mul<C>(c, r2), r2);
}
// the verdict on Montgomery evaluations: A B == C
template <class C> ZK_HD bool r1cs_holds(const Fp<C>& a, const Fp<C>& b, const Fp<C>& c) {
    const Fp<C> ab = r1cs_mul<C>(a, b);
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < C::N; i++) o |= ab.l[i] ^ c.l[i];
    return o == 0;
}

#if defined(__HIPCC__)
// ---- load -----------------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t R1CS_FLAG_SIGNAL = 1u;         // flags[0]: a term names a signal >= nVars
// combination of term t: the l with lc_first[l] <= t < lc_first[l + 1] (empty combinations repeat a value: the LAST index that is <= t)
ZK_DEV uint32_t r1cs_lc_of(const uint32_t* __restrict__ lc_first, uint32_t n_lc, uint32_t t) {
    uint32_t lo = 0, hi = n_lc;                   // invariant: lc_first[lo] <= t < lc_first[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (lc_first[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}
// word of the raw section at which term t of combination l starts: l + 1 counts and t records before it
ZK_DEV size_t r1cs_term_word(uint32_t l, uint32_t t) { return (size_t)l + 1 + 9 * (size_t)t; }
// place of term `rank` of row l in the sliced layout
ZK_DEV size_t r1cs_slot(uint32_t l, uint32_t rank, const uint32_t* __restrict__ seg_base, const uint32_t* __restrict__ pos_of_seg, const uint32_t* __restrict__ slice_off) {
    const uint32_t pos = pos_of_seg[seg_base[l] + rank / ABC_SEG];
    return ((size_t)slice_off[pos >> 6] + rank % ABC_SEG) * 64 + (pos & 63u);
}
static __global__ void k_r1cs_row_cnt(const uint32_t* __restrict__ lc_first, uint32_t rows, uint32_t* __restrict__ row_cnt) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < rows) row_cnt[r] = lc_first[r + 1] - lc_first[r];
}
// partial-sum slot -> index of its cut row in long_rows
static __global__ void k_r1cs_part_row(const uint32_t* __restrict__ long_rows, uint32_t n_long, uint32_t* __restrict__ part_row) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_long) return;
    const uint32_t pb = long_rows[3 * (size_t)k + 1], ns = long_rows[3 * (size_t)k + 2];
    for (uint32_t j = 0; j < ns; j++) part_row[pb + j] = k;
}
// one lane per TERM: its rank in the row comes from the prefix array, so no cursor is needed
template <class C> __global__ void __launch_bounds__(256)
k_r1cs_fill(const uint32_t* __restrict__ raw, const uint32_t* __restrict__ lc_first, uint32_t n_lc, uint32_t n_terms, uint32_t n_vars, const uint32_t* __restrict__ seg_base,
            const uint32_t* __restrict__ pos_of_seg, const uint32_t* __restrict__ slice_off, uint32_t* __restrict__ sell_sig, uint32_t* __restrict__ sell_val, uint32_t* __restrict__ flags) {
    const uint64_t t64 = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t64 >= n_terms) return;
    const uint32_t t = (uint32_t)t64, l = r1cs_lc_of(lc_first, n_lc, t);
    const uint32_t* rec = raw + r1cs_term_word(l, t);
    uint32_t s = rec[0];
    if (s >= n_vars) { atomicOr(flags, R1CS_FLAG_SIGNAL); s = 0; }
    Fp<C> c;
#pragma unroll
    for (int k = 0; k < 8; k++) c.l[k] = rec[1 + k];
    const size_t e = r1cs_slot(l, t - lc_first[l], seg_base, pos_of_seg, slice_off);
    sell_sig[e] = s;
    fp_store<C>(sell_val + e * 8, r1cs_coef<C>(c));
}
// marks the combinations whose signal ids are not strictly ascending: one adjacent compare per term
static __global__ void k_r1cs_dup_mark(const uint32_t* __restrict__ raw, const uint32_t* __restrict__ lc_first, uint32_t n_lc, uint32_t n_terms, uint32_t* __restrict__ marked,
                                       uint32_t* __restrict__ n_marked) {
    const uint64_t t64 = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t64 >= n_terms) return;
    const uint32_t t = (uint32_t)t64, l = r1cs_lc_of(lc_first, n_lc, t);
    if (t == lc_first[l]) return;
    const size_t w = r1cs_term_word(l, t);
    if (raw[w - 9] >= raw[w]) { marked[l] = 1u; atomicAdd(n_marked, 1u); }
}
// in the marked combinations only: a term that a later term of the combination repeats gets coefficient 0
static __global__ void k_r1cs_dup_fix(const uint32_t* __restrict__ raw, const uint32_t* __restrict__ lc_first, uint32_t n_lc, uint32_t n_terms, const uint32_t* __restrict__ marked,
                                      const uint32_t* __restrict__ seg_base, const uint32_t* __restrict__ pos_of_seg, const uint32_t* __restrict__ slice_off, uint32_t* __restrict__ sell_val) {
    const uint64_t t64 = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t64 >= n_terms) return;
    const uint32_t t = (uint32_t)t64, l = r1cs_lc_of(lc_first, n_lc, t);
    if (!marked[l]) return;
    const uint32_t s = raw[r1cs_term_word(l, t)], end = lc_first[l + 1];
    for (uint32_t u = t + 1; u < end; u++) {
        if (raw[r1cs_term_word(l, u)] != s) continue;
        const size_t e = r1cs_slot(l, t - lc_first[l], seg_base, pos_of_seg, slice_off);
        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
        reinterpret_cast<uint4*>(sell_val + e * 8)[0] = z; reinterpret_cast<uint4*>(sell_val + e * 8)[1] = z;
        return;
    }
}

// ---- check ----------------------------------------------------------------------------------------------------------------------------------
// witness values of any 256 bits -> below r
template <class C> __global__ void __launch_bounds__(256) k_r1cs_reduce_w(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t count) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    Fp<C> v = fp_load<C>(in + i * 8);
    r1cs_reduce256<C>(v);
    fp_store<C>(out + i * 8, v);
}
// The walk of k_abc_sell (groth16.hip) with blockIdx.y = witness, and the fold of the cut rows in the same launch: a segment of a cut row stores its
// partial sum, releases it (agent scope) and takes a ticket at the row's counter; the lane that takes the row's last ticket has every partial sum of the
// row behind its acquire, and its wave adds them up (lanes stride over the slots, then a shuffle tree), one such row after the other. Nothing waits.
// cnt: one counter per (witness, cut row), zeroed before every launch.
template <class C> __global__ void __launch_bounds__(256)
k_r1cs_sell(const uint32_t* __restrict__ s_len, const uint32_t* __restrict__ s_out, const uint32_t* __restrict__ slice_off, uint32_t n_seg, const uint32_t* __restrict__ sell_sig,
            const uint32_t* __restrict__ sell_val, const uint32_t* __restrict__ witness, uint32_t n_vars, uint32_t* ev, uint32_t rows, uint32_t* part, uint32_t n_part,
            const uint32_t* __restrict__ long_rows, uint32_t n_long, const uint32_t* __restrict__ part_row, uint32_t* cnt) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x, slice = p >> 6;
    if ((size_t)slice * 64 >= n_seg) return;                         // the whole wave
    const uint32_t* w_k = witness + (size_t)blockIdx.y * n_vars * 8;
    uint32_t* ev_k = ev + (size_t)blockIdx.y * rows * 8;
    uint32_t* part_k = part + (size_t)blockIdx.y * n_part * 8;
    const uint32_t width = __builtin_amdgcn_readfirstlane(s_len[(size_t)slice * 64]);
    const uint32_t len = p < n_seg ? s_len[p] : 0u;
    size_t e = (size_t)__builtin_amdgcn_readfirstlane(slice_off[slice]) * 64 + (p & 63u);
    Fp<C> acc = fp_zero<C>();
    for (uint32_t k = 0; k < width; k++, e += 64) {
        if (k < len) {
            const Fp<C> v = fp_load<C>(sell_val + e * 8);
            const Fp<C> w = fp_load<C>(w_k + (size_t)sell_sig[e] * 8);
            acc = fp_add(acc, fp_mul(v, w));
        }
    }
    const uint32_t o = p < n_seg ? s_out[p] : 0u;
    const bool cut = (o & ABC_PART) != 0;
    if (p < n_seg) fp_store<C>(cut ? part_k + (size_t)(o & ~ABC_PART) * 8 : ev_k + (size_t)o * 8, acc);
    if (!__any(cut)) return;                                         // wave-uniform from here on
    __threadfence();                                                 // release: this wave's partial sums, before its tickets
    uint32_t row_k = 0;
    bool last = false;
    if (cut) {
        row_k = part_row[o & ~ABC_PART];
        last = atomicAdd(&cnt[(size_t)blockIdx.y * n_long + row_k], 1u) + 1u == long_rows[3 * (size_t)row_k + 2];
    }
    unsigned long long todo = __ballot(last);
    if (!todo) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");               // acquire: the other waves' partial sums, after the last ticket
    const uint32_t lane = threadIdx.x & 63u;
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t kk = __shfl(row_k, leader);
        const uint32_t r = long_rows[3 * (size_t)kk], pb = long_rows[3 * (size_t)kk + 1], ns = long_rows[3 * (size_t)kk + 2];
        Fp<C> sum = fp_zero<C>();
        for (uint32_t j = lane; j < ns; j += 64) sum = fp_add(sum, fp_load<C>(part_k + (size_t)(pb + j) * 8));
        for (int off = 32; off; off >>= 1) {
            Fp<C> other;
#pragma unroll
            for (int i = 0; i < 8; i++) other.l[i] = __shfl_down(sum.l[i], off);
            sum = fp_add(sum, other);
        }
        if (lane == 0) fp_store<C>(ev_k + (size_t)r * 8, sum);
        todo &= todo - 1;
    }
}
// one lane per (witness, constraint): A B == C on the Montgomery evaluations; the smallest failing index of a wave goes into first_bad[witness] by one atomicMin
template <class C> __global__ void __launch_bounds__(256) k_r1cs_verdict(const uint32_t* __restrict__ ev, uint32_t n_constraints, uint32_t* __restrict__ first_bad) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    uint32_t bad = 0xffffffffu;
    if (c < n_constraints) {
        const uint32_t* row = ev + ((size_t)blockIdx.y * n_constraints * 3 + (size_t)c * 3) * 8;
        if (!r1cs_holds<C>(fp_load<C>(row), fp_load<C>(row + 8), fp_load<C>(row + 16))) bad = c;
    }
    for (int off = 32; off; off >>= 1) bad = min(bad, (uint32_t)__shfl_xor((int)bad, off));
    if ((threadIdx.x & 63u) == 0 && bad != 0xffffffffu) atomicMin(&first_bad[blockIdx.y], bad);
}
#endif  // __HIPCC__

}  // namespace zkmi
