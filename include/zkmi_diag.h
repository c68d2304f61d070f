/*
 * include/zkmi_diag.h — diagnostics of libzkmi.so: timing and statistics read-outs, calibration probes of the box a run landed on,
 * synthetic-base generators for tests and benchmarks, tuning knobs. None of these has a counterpart in the reference; bench.py, the
 * tests and tools/ use them, a snarkjs binding does not need them. The drop-in boundary is include/zkmi.h.
 *
 * Like the boundary itself the library is single-caller per process (zkmi.h, conventions): serialise these calls with the others.
 */
#ifndef ZKMI_DIAG_H
#define ZKMI_DIAG_H
#include "zkmi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* resident tables / their bytes / buffers seen once (no table yet) — for tests and diagnostics; any pointer may be NULL */
int zkmi_base_cache_stats(uint64_t* n_tables, uint64_t* table_bytes, uint64_t* n_seen);

/* Device time (ms, HIP events on the library stream) of the bucket-accumulation kernel of the last MSM that used job
 * slot `slot`: zkmi_msm / zkmi_msm_dev use slot 0; zkmi_groth16_prove uses 0..4 = A, B1, B2, C, H. -1 if never run. */
double zkmi_msm_accum_ms(int slot);
/* Diagnostics for the roofline accounting (bench.py int_alu): with zkmi_msm_stats(1) every bucket-accumulation launch is followed by a
 * small kernel that counts the mixed additions the launch performed (list entries of the digit sort whose base is not skipped and not the
 * point at infinity); zkmi_msm_accum_additions(slot) returns the count of the last MSM that used the job slot once the stream has been
 * synchronised (-1: never counted). Off by default; costs one pass over the sorted lists (~20 us at 2^20 terms) per MSM. */
int zkmi_msm_stats(int enable);
double zkmi_msm_accum_additions(int slot);

/* Window width used for n terms (tuning knob; 0 restores the built-in table). */
int zkmi_msm_set_window_bits(int c);

/* The front half of an MSM on its own, for tests: runs the digit sort and the lane schedule the product runs (csrc/msm_sort.hip: msm_sort, the
 * function behind every MSM entry point) over n device scalars of scalar_bytes bytes, waits for it, and copies what it built to the host.
 *   precomp_c     0: no window table — c bits per window as zkmi_msm_dev picks them (zkmi_msm_set_window_bits, else the built-in table for n) and one
 *                 set of buckets per window; 1..20: the lists of a window table built with that c (all windows share one set of buckets)
 *   table_stride  points per table row (0: n); only read with a table
 *   d_dropmask    optional device bitmap over the scalars, ceil(n / 32) words: a set bit leaves the scalar out of every list
 * What the sort chose comes back in *info (always written once the sort has run). The flat bucket index is g = window * nb + magnitude - 1 (window = 0 with a
 * table); a list entry is (table ? window * table_stride + i : i) | sign << 31 for scalar i.
 * Every output array may be NULL (not copied); one that is given must hold at least the stated number of words or the call fails with
 * ZKMI_ERR_INVALID — call once with NULL arrays to learn the sizes from *info:
 *   counts, starts   info->total words each, counts_cap words of room each: entries per bucket, and where the bucket's list begins in sorted
 *                    (the exclusive prefix sum of counts: the lists of all buckets form one flat array)
 *   sorted           info->entries words, sorted_cap of room: the lists, bucket after bucket; the order inside a bucket is arbitrary
 *   lane_g, lane_sub info->lanes words each, lanes_cap of room each: the bucket a lane of the accumulation works on, and which of the bucket's lanes it is
 *   giants           3 * info->giants words, 3 * giants_cap of room: (bucket, first lane >> 7, lanes >> 7) of every bucket with more than 128 lanes
 *   meta             3 words: all lanes, lanes of multi-lane buckets, giants
 * Same entry rules as zkmi_msm_dev: needs a device, refused while the active pipeline slot holds work in flight. */
typedef struct zkmi_msm_sort_info {
    uint32_t c, Wd, W;          /* window bits; digit windows of a scalar; sets of buckets (Wd, or 1 with a table) */
    uint32_t nb, total;         /* buckets per set = 2^(c-1); W * nb */
    uint32_t cap;               /* list entries per lane the schedule aims at */
    uint32_t nw;                /* 32-bit words of a scalar in the kernels instantiated for scalar_bytes: 1, 8 or 16 */
    uint32_t radix;             /* 1: two-level LDS radix sort; 0: counting sort on global atomics (every field down to chunks is 0 then) */
    uint32_t lb, parts;         /* radix: bits of the low key, and partitions = total >> lb */
    uint32_t fused_cap;         /* radix: a partition of at most this many pairs is finished by the fused level 2; 0: every partition is cut into chunks */
    uint32_t staged;            /* radix: 1 level-1 scatter ranked in LDS, 0 the direct scatter */
    uint32_t chunks;            /* radix: chunks (of at most 8 192 pairs) the chunked level 2 worked through */
    uint32_t entries;           /* list entries in all = non-zero digits of the scalars that were not dropped */
    uint32_t lanes, giants;     /* meta[0], meta[2] */
} zkmi_msm_sort_info;
int zkmi_msm_sort_probe_dev(const void* d_scalars, size_t n, size_t scalar_bytes, int precomp_c, size_t table_stride, const uint32_t* d_dropmask,
                            uint32_t* counts, uint32_t* starts, size_t counts_cap, uint32_t* sorted, size_t sorted_cap, uint32_t* lane_g, uint32_t* lane_sub,
                            size_t lanes_cap, uint32_t* giants, size_t giants_cap, uint32_t* meta, zkmi_msm_sort_info* info);

/* The back half of an MSM looked at from outside, for tests: runs ONE whole MSM through the product's own entry point and stages (msm_sort, then
 * csrc/msm_host.hpp: msm_accumulate with its k_msm_tree / k_msm_giant launches, msm_reduce, msm_fold), waits for it, and copies out what the stages left.
 *   table_handle  != 0: the MSM of zkmi_msm_table_dev over that table and the first n scalars (curve, group and d_bases are not read)
 *                 0: the MSM of zkmi_msm_dev over n caller-owned device bases, with its R'-form copy and the width of zkmi_msm_set_window_bits
 *   buckets       info->W * info->nb points, buckets_cap points of room: the finished buckets, g = window * nb + magnitude - 1 (window = 0 with a table);
 *                 a bucket without list entries is reported as the point at infinity (the reduction never reads its stale words)
 *   rowcol        2 * info->W << info->cbits points, rowcol_cap of room: the row and column sums in the order of msm_reduce's array,
 *                 ((window * 2 + kind) << cbits) + i with kind 0 = row i (infinity for i >= 2^rbits), 1 = column i; bucket = row << cbits | column
 *   result        the folded Jacobian point, as the entry point returns it (3 * group * n8q bytes)
 * Points leave in the format of the bases: affine, Montgomery form, all-zero for the point at infinity, whichever form the device kept them in.
 * Every output may be NULL (not copied); an array that is given and too small fails with ZKMI_ERR_INVALID after *info has been written — call once
 * with NULL arrays to learn the sizes. *info is written once the MSM has run. Same entry rules as the two entry points; in particular the call is
 * refused while the active pipeline slot holds work in flight. Product calls get no launch, copy or synchronisation for it: the picks are noted in host fields of the job. */
typedef struct zkmi_msm_stage_info {
    uint32_t c, W, nb;                   /* window bits; sets of buckets; buckets per set = 2^(c-1) */
    uint32_t rbits, cbits;               /* the bucket grid: 2^rbits rows of 2^cbits columns */
    uint32_t accum_kernel;               /* csrc/msm_select.hpp: MsmAccumKernel, 0 = accum29 ... 9 = accum32_wide */
    uint32_t rowcol_kernel;              /* csrc/msm_select.hpp: MsmRowcolKernel, 0 wave29, 1 wave29_compact, 2 wave29_g2, 3 wave, 4 staged */
    uint32_t r29_buckets;                /* 1: the finished buckets hold R'-form words */
    uint32_t bitsums;                    /* 1: the weighted sums ran as plain bit sums (k_msm_bitsums / _lds) and a Horner on the host, 0: k_msm_wsum */
    uint32_t cap;                        /* list entries per lane the schedule aimed at */
    uint32_t lanes, multi_lanes, giants; /* lanes in all, lanes of multi-lane buckets (k_msm_tree's input), buckets of more than 128 lanes (k_msm_giant's) */
} zkmi_msm_stage_info;
int zkmi_msm_stage_probe_dev(uint64_t table_handle, int curve, int group, const void* d_bases, const void* d_scalars, size_t n, size_t scalar_bytes, uint8_t* buckets,
                             size_t buckets_cap, uint8_t* rowcol, size_t rowcol_cap, uint8_t* result, zkmi_msm_stage_info* info);
/* Lanes per row / column sum of the last bucket reduction of `group` (1 | 2) in this process, whichever entry point ran it — an MSM, a batch of them, the
 * probe above, a proof: 8, 16, 32 or 64 for the row / column kernels on unsaturated limbs (rowcol_kernel 0, 1, 2: csrc/msm_select.hpp picks the count from
 * the launch's shape, or ZKMI_RC_LANES for G1 and ZKMI_RC_LANES_G2 for G2 force it; any other value of a switch makes the reduction fail with
 * ZKMI_ERR_INVALID), 64 for the generic wave kernel (3), 0 for the staged sums (4) or when the group has not reduced anything yet; -1 for another group.
 * The info record of the probe does not carry it: its layout is fixed. Host only: a field the driver notes, no launch, copy or synchronisation. */
int zkmi_msm_rowcol_lanes(int group);

/* Device time (ms, HIP events) of the stages of the last proof, in order: buildABC, 6 NTTs, joinABC, sort(witness),
 * bucket accumulation of MSM B2, B1 (+ the second witness sort), A, C, sort(H scalars), accumulation of MSM H, batched G1 bucket reductions (the B2
 * reduction runs on a second stream underneath the G1 accumulations).
 * Writes min(n, ZKMI_GROTH16_STAGES) values. */
#define ZKMI_GROTH16_STAGES 11
int zkmi_groth16_stage_ms(double* out, int n);

/* Two short probes of the device a run landed on, for reading benchmark lines (no reference counterpart): Montgomery products per second on
 * 29-bit limbs (two dependent chains per lane, 8 workgroups per CU: about 150 G products/s on a healthy MI355X) and 16 dependent random 128-byte
 * gathers per lane over a 2 GiB table (about 6 TB/s on a healthy box). */
int zkmi_calibrate_box(double* mul29_gmul_per_s, double* gather128_gb_per_s);
/* Third probe: the same product chain as straight-line loops of ~17 KB and ~210 KB of code at two waves per SIMD; big / small < 1 is the cost of
 * instruction fetch beyond the 64 KB instruction cache on this box (the accumulation loops of the 14-limb curve are that large). */
int zkmi_calibrate_code_fetch(double* small_loop_gmul_per_s, double* big_loop_gmul_per_s);
/* Which MSM kernels run their compact instantiation (products called instead of inlined: loops that fit the instruction cache) on this box:
 * bit 0 G1 accumulation of the 14-limb curve, 1 its G2 accumulation, 2 G1 row/column sums, 3 Fq2 row/column sums by the generic kernel, 4 PLONK's quotient
 * numerator by the 32-bit kernels with called products; decided once from the probe above — bits 1, 2, 3 when big / small < 0.85 (r05: the loops behind bits 0
 * and 4 fit the instruction cache since r04 and measured faster inlined on such a box) — unless ZKMI_COMPACT_CODE=<mask> is set. Results are bit-identical
 * either way. -1: no device. */
int zkmi_compact_code(void);

/* How zkmi_ntt* would run a transform of 2^log_n points in THIS process: *n_pass = the passes over the array (1..4), l[0..4) = the digit widths of the
 * passes, most significant input digit first (they sum to log_n; unused entries 0), *limbs29 = 1 when the passes run on 9 x 29-bit limbs (csrc/ntt29.cuh),
 * 0 on saturated 32-bit limbs (csrc/ntt.cuh). The answer comes from the functions the driver itself decides with (csrc/ntt_plan.hpp) and follows the
 * switches it reads once per process: ZKMI_NTT_DIGIT (bits per digit at most, default 8: one pass up to 2^9, two up to 2^16, three up to 2^24, four from
 * 2^25 to Fr.s), ZKMI_NTT29 and ZKMI_NTT29_MAX_LOG. Fails as the transform would, with ZKMI_ERR_UNSUPPORTED: log_n above Fr.s, or a digit cap under which
 * 2^log_n would need more than four passes (or a cap outside 1..9); the outputs are not written then. Host only, needs no device; any output may be NULL. */
int zkmi_ntt_plan_probe(int curve, unsigned log_n, uint32_t* n_pass, uint32_t l[4], int* limbs29);

/* Synthetic base table of SURVEY.md §8d: P_i = (f*g^i mod r)*G written to device memory as affine Montgomery points
 * (what G.batchApplyKey(G repeated n, Fr.e(f), Fr.e(g)) returns).  For benchmarks and tests. */
int zkmi_gen_geometric_bases_dev(int curve, int group, size_t n, uint64_t f, uint64_t g, void* d_out);
/* P_i = k_i * G for n caller-supplied scalars (device, 32-byte little-endian integers, normal form), affine Montgomery points out:
 * the base sections of synthetic VALID proving keys built from a known trapdoor (src/zkey_new.js:182-201, :338-502
 * compute the same points from a ptau file). For tests and benchmarks. */
int zkmi_gen_bases_from_scalars_dev(int curve, int group, const void* d_scalars, size_t n, void* d_out);

/* Wall-clock-free device timing of the last call of each kind, in milliseconds (HIP events on the library stream). */
double zkmi_last_kernel_ms(void);
/* zkmi_msm_dev calls since start-up that ran on the saturated-limb path because the scratch copy of the bases (n x 2*group*n8q bytes) could not be allocated
 * (out of memory ONLY: any other failure is reported by the call itself). A non-zero count explains a slow standalone MSM. */
unsigned long long zkmi_msm_dev_fallbacks(void);
/* Shape of the resident coefficient layout of a Groth16 key (csrc/groth16.hip: buildABC as a length-sorted sliced layout with split rows):
 * out[0..5) = coefficient records, segments (<= 32 terms each), rows cut into several segments, partial-sum slots, padded terms held. */
int zkmi_groth16_coef_layout(uint64_t zkey_cache_key, uint64_t* out, int n);

/* Reduced pairing e(P_i, Q_i) (the curve.pairing of ffjavascript that src/groth16_verify.js:66-74 compares through pairingEq) of n pairs,
 * for tests and debugging: g1_xyz n x 3 Fq, g2_xyz n x 3 Fq2 in the (x, y, z) form of zkmi_groth16_vk_load; out_f12 n x 12 Fq, standard form,
 * the coefficients of w^0..w^11 in Fq[w]/(w^12 - 2s w^6 + s^2 + 1), xi = s + u (oracle/groth16_verify_oracle.py). A point at infinity gives 1. */
int zkmi_pairing_dev(int curve, const uint8_t* g1_xyz, const uint8_t* g2_xyz, size_t n, uint8_t* out_f12);
/* Device time of the verification kernel of the last zkmi_groth16_verify_batch, in milliseconds (HIP events on the verifier's stream); -1: none yet.
 * After an aggregated batch: its three phases together. */
double zkmi_groth16_verify_last_ms(void);
/* The intermediate values of the PLONK verifier for ONE proof (inputs as zkmi_plonk_verify_batch with n = 1), so that a wrong verdict can be
 * located: out = beta gamma alpha xi v1 u L1(xi) PI(xi) r0 (9 x 32 bytes, Fr, standard form) | A1.x A1.y B1.x B1.y (n8q bytes each, affine,
 * standard form, the point at infinity all-zero): 288 + 4 n8q bytes. All-zero for a proof that fails the input checks. */
int zkmi_plonk_verify_trace_dev(uint64_t vk_handle, const uint8_t* proof, const uint8_t* publics, uint32_t n_signals, uint8_t* out);
/* Device time of the verification kernel of the last zkmi_plonk_verify_batch, in milliseconds; -1: none yet. */
double zkmi_plonk_verify_last_ms(void);
/* The intermediate values of the FFLONK verifier for ONE proof (inputs as zkmi_fflonk_verify_batch with n = 1): out = beta gamma xi alpha y r0
 * r1 r2 (8 x 32 bytes, Fr, standard form) | A1.x A1.y B1.x B1.y (n8q bytes each, affine, standard form, the point at infinity all-zero; B1 is
 * W2): 256 + 4 n8q bytes. All-zero for a proof that fails the input checks. */
int zkmi_fflonk_verify_trace_dev(uint64_t vk_handle, const uint8_t* proof, const uint8_t* publics, uint32_t n_signals, uint8_t* out);
/* Device time of the verification kernel of the last zkmi_fflonk_verify_batch, in milliseconds; -1: none yet. */
double zkmi_fflonk_verify_last_ms(void);
/* zkmi_*_verify_aggregate with its two sums reported: sums = S_P.x S_P.y S_Q.x S_Q.y (n8q bytes each, affine, standard form, before the cofactor
 * multiplication; the point at infinity all-zero): 4 n8q bytes. */
int zkmi_plonk_aggregate_trace_dev(uint64_t vk_handle, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, const uint8_t seed[32], int8_t* codes,
                                   int* ok, uint8_t* sums);
int zkmi_fflonk_aggregate_trace_dev(uint64_t vk_handle, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, const uint8_t seed[32], int8_t* codes,
                                    int* ok, uint8_t* sums);
/* Device time of the lane phase | the reduction | the tail of the last aggregated batch, in milliseconds (three doubles; -1 where the verifier's
 * last batch was not an aggregated one). After an aggregated batch zkmi_*_verify_last_ms reports the three together. */
int zkmi_plonk_aggregate_phase_ms(double* lane_reduce_tail);
int zkmi_fflonk_aggregate_phase_ms(double* lane_reduce_tail);
/* zkmi_groth16_verify_aggregate with its intermediate values reported: trace = S_X.x S_X.y S_C.x S_C.y (n8q bytes each, affine, standard form,
 * before the cofactor multiplication; the point at infinity all-zero) | s = sum r_i (24 bytes, little-endian) | final_exp(F), the plain final
 * exponentiation of the product of the lanes' Miller values, as 12 Fq in the w-basis of zkmi_pairing_dev: 16 n8q + 24 bytes. */
int zkmi_groth16_aggregate_trace_dev(uint64_t vk_handle, const uint8_t* proofs_xyz, const uint8_t* publics, uint32_t n_signals, size_t n, const uint8_t seed[32], int8_t* codes,
                                     int* ok, uint8_t* trace);
/* lane phase | reduction | tail of the Groth16 verifier's last batch when it was an aggregated one (-1 each otherwise), as above */
int zkmi_groth16_aggregate_phase_ms(double* lane_reduce_tail);
/* Device time in ms of the last zkmi_groth16_setup, five values: the evaluate + fold + to-affine launches of A, B1, B2 and IC|C, then the H differences. */
int zkmi_groth16_setup_phase_ms(double* out5);
/* Wall time in ms of the last PLONK setup, four values: the gate lowering on the host (the last zkmi_plonk_setup_lower or _lower_len), then of the last
 * zkmi_plonk_setup the selector padding and sigma, writeP4 for the eight columns and the Lagrange section, the table build and the eight commitments. */
int zkmi_plonk_setup_phase_ms(double* out4);
/* Wall time in ms of the last FFLONK setup, four values: the gate lowering on the host (the last zkmi_fflonk_setup_lower or _lower_len), then of the
 * last zkmi_fflonk_setup the selector padding and sigma, the transforms of the eight columns and the Lagrange section, the C0 kernel and its commitment. */
int zkmi_fflonk_setup_phase_ms(double* out4);
/* The digit stream zkmi_group_scale hands its kernel for the scalar k (Montgomery Fr): the non-adjacent form of k, most significant digit first, one
 * digit (-1, 0, 1) per byte; digits holds at least 256 bytes, *n_digits receives the count (0 for k = 0). Host only, needs no device. */
int zkmi_group_scale_recode(int curve, const uint8_t* k_mont, int8_t* digits, int* n_digits);
/* What the generator kernels of zkmi_chacha_words_dev / zkmi_chacha_fr_dev are held to (csrc/chacha.cuh, csrc/phase2_host.hpp). Host only, no device.
 *   _block_host         the block function the kernels run, on the host: block (counter_hi << 64 | counter_lo) of the keystream, 16 words
 *   _struct_words_host  the same words drawn from the sequential generator struct (the pinned restatement), its counter set to block first_word / 16
 *   _fr_host            n sequential Fr.fromRng draws from that struct (32 bytes each) and the position it ends at
 *   _fr_compact_host    the kernels' rule on the host: attempts through the block function, kept ones in order
 * zkmi_chacha_set_round_blocks: keystream blocks per round of zkmi_chacha_fr_dev (0, the default: by the curve's keep rate); the result does not depend on it. */
int zkmi_chacha_block_host(const uint32_t seed8[8], uint64_t counter_lo, uint64_t counter_hi, uint32_t* out16);
int zkmi_chacha_struct_words_host(const uint32_t seed8[8], uint64_t first_word, uint32_t* out, size_t n_words);
int zkmi_chacha_fr_host(int curve, const uint32_t seed8[8], uint8_t* out, size_t n, uint64_t* words_consumed);
int zkmi_chacha_fr_compact_host(int curve, const uint32_t seed8[8], uint8_t* out, size_t n, uint64_t* words_consumed);
int zkmi_chacha_set_round_blocks(size_t blocks);
/* The G1 kernel of zkmi_ptau_contribute_section on its own (csrc/ptau_contribute.cuh): out_i = k_i * P_i for n affine LEM points and n scalars of 32 bytes,
 * little-endian, normal form, below 2^255 (device pointers; d_out must not overlap d_points). group must be 1: group 2 returns ZKMI_ERR_UNSUPPORTED, it has no
 * such kernel (the group argument is there for that refusal alone). Refused while a pipeline slot holds work in flight. Like every _dev entry the call only
 * enqueues on the library stream and returns: d_out is complete once that stream has drained (zkmi_synchronize, or any later library call or zkmi_memcpy_d2h, which
 * are ordered behind it). Scalars of r and above are taken as they are: the digits are read from the bits, so k P comes out for every k below 2^255.
 * zkmi_diag_set_ptau_slice: points per slice of zkmi_ptau_contribute_section (0 restores the default of 2^20); the result does not depend on it. */
int zkmi_diag_group_mul_each_dev(int curve, int group, const void* d_points, const void* d_scalars_normal, void* d_out, size_t n);
int zkmi_diag_set_ptau_slice(size_t points);
/* The G2 kernel of zkmi_ptau_challenge_section on its own (csrc/ptau_challenge.cuh): out_i = k_i * P_i for n affine LEM points of G2 (or of the twist outside
 * it) and n scalars as above (device pointers; d_out must not overlap d_points). The refusals of zkmi_diag_group_mul_each_dev, in its words; it only enqueues
 * on the library stream. For a point of order r every k below 2^255 gives (k mod r) P_i. */
int zkmi_diag_group2_mul_each_dev(int curve, const void* d_points, const void* d_scalars_normal, void* d_out, size_t n);
/* Bytes of work memory one pass of zkmi_r1cs_check(_dev) may take (0 restores the default of 4 GiB): a batch of witnesses is cut into passes that fit, one
 * witness at the least; the verdicts do not depend on it. */
int zkmi_diag_set_r1cs_budget(size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* ZKMI_DIAG_H */
