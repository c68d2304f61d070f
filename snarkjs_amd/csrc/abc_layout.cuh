// snarkjs_amd/csrc/abc_layout.cuh — the witness-independent kernels of the sliced-ELL layout with split rows that groth16.hip builds from zkey section 4
// (rows = (matrix, constraint) of A | B) and r1cs_check.hip builds from r1cs section 2 (rows = 3 * constraint + matrix of A, B, C). The layout itself is
// described at the head of groth16.hip; what is here turns per-row term counts into sorted segments, slices and partial-sum slots. Filling the terms in and
// walking them with a witness are each unit's own kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace zkmi {

constexpr uint32_t ABC_SEG = 32;                 // terms per segment: a slice of full width is 32 dependent product-accumulates per lane
constexpr uint32_t ABC_PART = 0x80000000u;       // s_out: the segment writes partial sum (s_out & ~ABC_PART) instead of row s_out
// exclusive scan of `n` counters by one workgroup (one-off per zkey); out must not alias in
static __global__ void k_scan_u32(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    __shared__ uint32_t part[1024];
    const uint32_t per = (n + blockDim.x - 1) / blockDim.x;
    const uint32_t lo = min(n, threadIdx.x * per), hi = min(n, lo + per);
    uint32_t sum = 0;
    for (uint32_t b = lo; b < hi; b++) sum += in[b];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < blockDim.x; d <<= 1) {
        uint32_t v = threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;
    for (uint32_t b = lo; b < hi; b++) { out[b] = run; run += in[b]; }
}
// per row: its number of segments and, for rows cut into several, of partial-sum slots
static __global__ void k_abc_row_segs(const uint32_t* __restrict__ row_cnt, uint32_t rows, uint32_t* __restrict__ nseg, uint32_t* __restrict__ npart) {
    uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const uint32_t c = row_cnt[r], ns = c ? (c + ABC_SEG - 1) / ABC_SEG : 1u;
    nseg[r] = ns;
    npart[r] = ns > 1 ? ns : 0u;
}
// one lane per row: lengths and targets of its segments; cut rows join the list of long rows (row, first partial slot, segments)
static __global__ void k_abc_seg_fill(const uint32_t* __restrict__ row_cnt, const uint32_t* __restrict__ seg_base, const uint32_t* __restrict__ part_base, uint32_t rows,
                                      uint32_t* __restrict__ seg_len, uint32_t* __restrict__ seg_out, uint32_t* __restrict__ long_rows, uint32_t* __restrict__ n_long) {
    uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const uint32_t c = row_cnt[r], sb = seg_base[r];
    if (c <= ABC_SEG) { seg_len[sb] = c; seg_out[sb] = r; return; }
    const uint32_t ns = (c + ABC_SEG - 1) / ABC_SEG, pb = part_base[r];
    for (uint32_t j = 0; j < ns; j++) { seg_len[sb + j] = min(ABC_SEG, c - j * ABC_SEG); seg_out[sb + j] = ABC_PART | (pb + j); }
    const uint32_t k = atomicAdd(n_long, 1u);
    long_rows[3 * (size_t)k] = r; long_rows[3 * (size_t)k + 1] = pb; long_rows[3 * (size_t)k + 2] = ns;
}
// Stable counting sort of the segments by length, longest first. One wave per 64 segments (blockDim = 64): the lanes that share a length are found
// by ballots; counts[(ABC_SEG - len) * n_waves + wave] = their number. One flat exclusive scan over that [bin][wave] array is every (bin, wave)'s
// first position in the sorted order; the rank inside the wave is the number of lower lanes of the same length.
static __global__ void __launch_bounds__(64) k_abc_wave_hist(const uint32_t* __restrict__ seg_len, uint32_t n_seg, uint32_t n_waves, uint32_t* __restrict__ counts) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    const bool live = s < n_seg;
    const uint32_t len = live ? seg_len[s] : 0xffffffffu;
    unsigned long long todo = __ballot(live);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t v = __shfl(len, leader);
        const unsigned long long same = __ballot(live && len == v);
        if ((int)threadIdx.x == leader) counts[(size_t)(ABC_SEG - v) * n_waves + blockIdx.x] = (uint32_t)__popcll(same);
        todo &= ~same;
    }
}
static __global__ void __launch_bounds__(64) k_abc_wave_rank(const uint32_t* __restrict__ seg_len, const uint32_t* __restrict__ seg_out, uint32_t n_seg, uint32_t n_waves,
                                                            const uint32_t* __restrict__ offs, uint32_t* __restrict__ s_len, uint32_t* __restrict__ s_out, uint32_t* __restrict__ pos_of_seg) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    const bool live = s < n_seg;
    const uint32_t len = live ? seg_len[s] : 0xffffffffu;
    unsigned long long todo = __ballot(live);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t v = __shfl(len, leader);
        const unsigned long long same = __ballot(live && len == v);
        if (live && len == v) {
            const uint32_t pos = offs[(size_t)(ABC_SEG - v) * n_waves + blockIdx.x] + (uint32_t)__popcll(same & ((1ull << threadIdx.x) - 1ull));
            s_len[pos] = len; s_out[pos] = seg_out[s]; pos_of_seg[s] = pos;
        }
        todo &= ~same;
    }
}
static __global__ void k_abc_slice_w(const uint32_t* __restrict__ s_len, uint32_t n_slices, uint32_t* __restrict__ slice_w) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_slices) slice_w[i] = s_len[(size_t)i * 64];       // sorted longest first: the slice's first segment is its widest
}

}  // namespace zkmi
