// snarkjs_amd/csrc/chacha.cuh — the reference's deterministic generator (ffjavascript's ChaCha) and its Fr.fromRng, position by position.
//
// phase2::ChaCha (phase2_host.hpp) is the sequential restatement the golden vectors pin. A sequential generator is a loop; the keystream itself is not:
// block k depends on (seed, k) alone. chacha::block computes one block from the seed and the 128-bit block counter, for the host and the device alike;
// the host struct stays what it was and this function is held to it (tests/test_phase2_verify_host.py).
//   block       constants in words 0 - 3, the seed in 4 - 11, the counter in 12 - 15 (little end in 12, carries upwards), 20 rounds, the input added
//   candidate   Fr.fromRng reads n64 = 4 nextU64 per attempt, each nextU64 two nextU32 with the HIGH half first: attempt k is words 8k .. 8k + 7 of the
//               keystream, limb i = w[2i] << 32 | w[2i + 1], masked to the bit length of r, kept iff < r. A block is two attempts.
// Fr.fromRng draws until an attempt is kept, so the i-th value of a fresh generator is the i-th kept attempt: one lane per block flags its two attempts,
// an exclusive scan of the flags gives every kept attempt its place, and a second pass writes it there. No atomic decides a place.
//   k_chacha_words       one lane per block; the 16 words of the 256 blocks of a workgroup cross LDS (row stride 17, conflict-free both ways) so that
//                        the stores are consecutive dwords from consecutive lanes whatever first_word is
//   k_chacha_fr_count    per workgroup: how many of its 512 attempts are kept
//   k_chacha_scan        one workgroup: exclusive scan of those counts, and their total
//   k_chacha_fr_scatter  recomputes the block (320 adds, xors and rotates: cheaper than keeping 64 bytes per lane between the passes), scans the 256
//                        counts of the workgroup in LDS and writes the kept attempts to their places below n
// The rotate is __builtin_rotateleft32: one v_alignbit_b32 on the device, a rol on the host.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace zkmi {
namespace chacha {

#define ZK_CHACHA_HD __host__ __device__ __forceinline__

struct Seed { uint32_t w[8]; };

ZK_CHACHA_HD void quarter(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
    a += b; d = __builtin_rotateleft32(d ^ a, 16);
    c += d; b = __builtin_rotateleft32(b ^ c, 12);
    a += b; d = __builtin_rotateleft32(d ^ a, 8);
    c += d; b = __builtin_rotateleft32(b ^ c, 7);
}

// block (ctr_hi << 64 | ctr_lo) of the keystream of `seed`, in nextU32 order
ZK_CHACHA_HD void block(const uint32_t* seed, uint64_t ctr_lo, uint64_t ctr_hi, uint32_t* out) {
    uint32_t s[16], x[16];
    s[0] = 0x61707865u; s[1] = 0x3320646eu; s[2] = 0x79622d32u; s[3] = 0x6b206574u;
#pragma unroll
    for (int i = 0; i < 8; i++) s[4 + i] = seed[i];
    s[12] = (uint32_t)ctr_lo; s[13] = (uint32_t)(ctr_lo >> 32); s[14] = (uint32_t)ctr_hi; s[15] = (uint32_t)(ctr_hi >> 32);
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = s[i];
#pragma unroll
    for (int r = 0; r < 10; r++) {
        quarter(x[0], x[4], x[8], x[12]); quarter(x[1], x[5], x[9], x[13]); quarter(x[2], x[6], x[10], x[14]); quarter(x[3], x[7], x[11], x[15]);
        quarter(x[0], x[5], x[10], x[15]); quarter(x[1], x[6], x[11], x[12]); quarter(x[2], x[7], x[8], x[13]); quarter(x[3], x[4], x[9], x[14]);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] = x[i] + s[i];
}

// bit length of the modulus of FrC (8 words): 254 (BN254), 255 (BLS12-381)
template <class FrC> ZK_CHACHA_HD constexpr int modulus_bits() {
    int b = 0;
    for (int i = 0; i < 32; i++) if ((FrC::p(7) >> i) & 1u) b = i + 1;
    return 224 + b;
}

// One attempt of Fr.fromRng from eight keystream words: the masked integer as eight little-endian 32-bit words; true iff it is below r.
template <class FrC> ZK_CHACHA_HD bool candidate(const uint32_t* w, uint32_t* out) {
    static_assert(FrC::N == 8, "Fr has n64 = 4 on both curves");
    constexpr int top = modulus_bits<FrC>() - 224;
#pragma unroll
    for (int i = 0; i < 4; i++) { out[2 * i] = w[2 * i + 1]; out[2 * i + 1] = w[2 * i]; }
    if (top < 32) out[7] &= (1u << top) - 1u;
    // out < r: the borrow of out - r
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t d = (uint64_t)out[i] - FrC::p(i) - borrow;
        borrow = (uint32_t)(d >> 63);
    }
    return borrow != 0;
}

constexpr int T = 256;          // lanes (= keystream blocks) per workgroup of every kernel here

#if defined(__HIPCC__) && !defined(ZKMI_CHACHA_NO_KERNELS)          // tools/chacha_hosttest.hip: the host pass alone, no code object to register
// out[j] = keystream word first_word + j, j < n_words; workgroup g holds blocks first_word / 16 + 256 g ..
__global__ void __launch_bounds__(T) k_chacha_words(Seed seed, uint64_t first_word, uint32_t* __restrict__ out, uint64_t n_words) {
    __shared__ uint32_t lds[T * 17];
    const uint64_t b0 = first_word / 16 + (uint64_t)blockIdx.x * T;
    uint32_t w[16];
    block(seed.w, b0 + threadIdx.x, 0, w);
#pragma unroll
    for (int i = 0; i < 16; i++) lds[threadIdx.x * 17 + i] = w[i];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t v = k * T + threadIdx.x;                          // word of the workgroup
        const uint64_t W = b0 * 16 + v;                                   // word of the stream
        if (W >= first_word && W - first_word < n_words) out[W - first_word] = lds[(v >> 4) * 17 + (v & 15)];
    }
}

// the two attempts of block `b`: their masked integers and bit k of the result set iff attempt k is kept
template <class FrC> __device__ __forceinline__ uint32_t attempts_of(const Seed& seed, uint64_t b, uint32_t* c0, uint32_t* c1) {
    uint32_t w[16];
    block(seed.w, b, 0, w);
    return (candidate<FrC>(w, c0) ? 1u : 0u) | (candidate<FrC>(w + 8, c1) ? 2u : 0u);
}

// sum over the workgroup (every lane calls it; the result is valid in every lane)
__device__ __forceinline__ uint32_t wg_sum(uint32_t v, uint32_t* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = T / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

// wg_kept[g] = kept attempts among blocks first_block + 256 g .. (blocks at or beyond n_blocks count nothing)
template <class FrC> __global__ void __launch_bounds__(T) k_chacha_fr_count(Seed seed, uint64_t first_block, uint32_t n_blocks, uint32_t* __restrict__ wg_kept) {
    __shared__ uint32_t sh[T];
    const uint32_t i = blockIdx.x * T + threadIdx.x;
    uint32_t c0[8], c1[8], cnt = 0;
    if (i < n_blocks) cnt = __builtin_popcount(attempts_of<FrC>(seed, first_block + i, c0, c1));
    const uint32_t total = wg_sum(cnt, sh);
    if (threadIdx.x == 0) wg_kept[blockIdx.x] = total;
}

// in place: v[g] <- sum of v[0 .. g); *total <- the sum of all n_wg entries. ONE workgroup: lane t owns a contiguous run of entries.
__global__ void __launch_bounds__(T) k_chacha_scan(uint32_t* __restrict__ v, uint32_t n_wg, uint32_t* __restrict__ total) {
    __shared__ uint32_t sh[T];
    const uint32_t per = (n_wg + T - 1) / T;
    const uint32_t lo = threadIdx.x * per < n_wg ? threadIdx.x * per : n_wg, hi = lo + per < n_wg ? lo + per : n_wg;
    uint32_t s = 0;
    for (uint32_t k = lo; k < hi; k++) s += v[k];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int t = 0; t < T; t++) { const uint32_t c = sh[t]; sh[t] = run; run += c; }
        *total = run;
    }
    __syncthreads();
    uint32_t run = sh[threadIdx.x];
    for (uint32_t k = lo; k < hi; k++) { const uint32_t c = v[k]; v[k] = run; run += c; }
}

// the kept attempts of blocks first_block .. + n_blocks to out[base + place], place by the scan, for every place below n; the lane that writes place
// n - 1 also writes the index of that attempt (2 block + k) to *last_attempt
template <class FrC> __global__ void __launch_bounds__(T) k_chacha_fr_scatter(Seed seed, uint64_t first_block, uint32_t n_blocks, const uint32_t* __restrict__ wg_off,
                                                                               uint64_t base, uint64_t n, uint32_t* __restrict__ out, uint64_t* __restrict__ last_attempt) {
    __shared__ uint32_t sh[T];
    const uint32_t i = blockIdx.x * T + threadIdx.x;
    uint32_t c0[8], c1[8], keep = 0;
    if (i < n_blocks) keep = attempts_of<FrC>(seed, first_block + i, c0, c1);
    const uint32_t cnt = __builtin_popcount(keep);
    // exclusive scan of the 256 counts (Hillis - Steele on the inclusive sums)
    sh[threadIdx.x] = cnt;
    __syncthreads();
    for (int d = 1; d < T; d <<= 1) {
        const uint32_t add = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0u;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    uint64_t place = base + wg_off[blockIdx.x] + (sh[threadIdx.x] - cnt);
#pragma unroll
    for (int k = 0; k < 2; k++) {
        if (!((keep >> k) & 1u)) continue;
        if (place < n) {
            const uint32_t* c = k ? c1 : c0;
            uint4* dst = (uint4*)(out + place * 8);
            dst[0] = make_uint4(c[0], c[1], c[2], c[3]);
            dst[1] = make_uint4(c[4], c[5], c[6], c[7]);
            if (place == n - 1) *last_attempt = 2 * (first_block + i) + k;
        }
        place++;
    }
}
#endif  // kernels

// The same rule on the host, attempt by attempt through `block` and `candidate` (not through phase2::ChaCha): the first n kept attempts as 32-byte
// little-endian integers; returns the position a sequential generator would be at.
template <class FrC> inline uint64_t fr_stream_host(const uint32_t* seed, uint8_t* out, size_t n) {
    uint64_t b = 0, words = 0;
    size_t got = 0;
    while (got < n) {
        uint32_t w[16], c[8];
        block(seed, b, 0, w);
        for (int k = 0; k < 2 && got < n; k++) {
            const bool keep = candidate<FrC>(w + 8 * k, c);
            words = 16 * b + 8 * (k + 1);
            if (!keep) continue;
            for (int i = 0; i < 8; i++) for (int j = 0; j < 4; j++) out[got * 32 + 4 * i + j] = (uint8_t)(c[i] >> (8 * j));
            got++;
        }
        b++;
    }
    return words;
}

}  // namespace chacha
}  // namespace zkmi
