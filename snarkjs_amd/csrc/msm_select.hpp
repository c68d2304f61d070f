// snarkjs_amd/csrc/msm_select.hpp — which MSM kernel runs. The A/B switches of the MSM host driver (msm_host.hpp) and the two pure functions
// that turn (group, limb form, table form, window width, box, switches) into a kernel and its launch shape. Plain C++17 without a HIP header:
// tools/msm_select_hosttest.hip compiles it for the host and tests/test_msm_select_host.py pins every rule below. DESIGN.md §4.2 has the table
// of the switches.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/zkmi.h"

namespace zkmi {

// Read once per process. A boolean switch is off only when its variable is set and atoi() of it is 0.
struct MsmTuning {
    bool rowcol_wave = true;        // one wave per row / column sum with the fold inside the launch; off: the staged k_msm_rowcol + k_msm_fold sequence
    bool r29_reduce = true;         // G1 buckets leave the accumulation in R'-form and k_msm_rowcol_wave29 reduces them; off: R-form and the generic sums
    bool r29_reduce_g2 = true;      // the same for the Fq2 buckets (k_msm_rowcol_wave29_g2)
    int acc29_block = 0;            // threads per block of the G1 29-bit accumulation; honoured for 64, 128 and 256 only
    bool g2_split = true;           // G2 accumulation with one Fq2 component per lane (k_msm_accum29_g2s); off: the LDS-parked layouts
    bool g2_split_bls = true;       // off: the 14-limb curve alone goes back to the LDS-parked layout
    int aux_rc_sums = 512;          // row / column sums (waves) in flight on the auxiliary stream; <= 0: no cap
    bool multi_overlap = true;      // msm_table_multi: the digit sorts on the auxiliary stream, underneath the previous accumulation
    int rc_lanes = 0;               // lanes per row / column sum of k_msm_rowcol_wave29: 8, 16, 32 or 64; 0 (not set): msm_rowcol_pick's own choice
    int rc_lanes_g2 = 0;            // the same for k_msm_rowcol_wave29_g2
};
inline const MsmTuning& msm_tuning() {
    static const MsmTuning t = [] {
        auto on = [](const char* name) { const char* e = getenv(name); return !(e && atoi(e) == 0); };
        auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
        MsmTuning v;
        v.rowcol_wave = on("ZKMI_ROWCOL_WAVE");
        v.r29_reduce = on("ZKMI_R29_REDUCE");
        v.r29_reduce_g2 = on("ZKMI_R29_REDUCE_G2");
        v.acc29_block = num("ZKMI_ACC29_BLOCK", 0);
        v.g2_split = on("ZKMI_G2_SPLIT");
        v.g2_split_bls = on("ZKMI_G2_SPLIT_BLS");
        v.aux_rc_sums = num("ZKMI_AUX_RC_SUMS", 512);
        v.multi_overlap = on("ZKMI_MULTI_OVERLAP");
        // set to something that is no number, or to 0: -1, which the pick refuses like any other value that is not a lane count
        auto lanes = [](const char* name) { const char* e = getenv(name); return !e ? 0 : atoi(e) ? atoi(e) : -1; };
        v.rc_lanes = lanes("ZKMI_RC_LANES");
        v.rc_lanes_g2 = lanes("ZKMI_RC_LANES_G2");
        return v;
    }();
    return t;
}

// One name per kernel instantiation the drivers launch (F = the group's field over the curve C).
enum class MsmAccumKernel {
    accum29, accum29_merge, accum29_compact, accum29_compact_merge,      // k_msm_accum29<C | Compact<C>, merge>
    accum29_g2s,                                                         // k_msm_accum29_g2s<C>
    accum29_g2, accum29_g2_compact,                                      // k_msm_accum29_g2<C | Compact<C>>
    accum32, accum32_merge, accum32_wide                                 // k_msm_accum<F, false, false | true>, k_msm_accum<F, true, false>
};
enum class MsmRowcolKernel { wave29, wave29_compact, wave29_g2, wave, staged };
enum class MsmPickError { none, merge_g2, merge_r29_target, r29_needs_wave, rc_lanes };
inline int msm_pick_code(MsmPickError e) {
    return e == MsmPickError::none ? ZKMI_OK : (e == MsmPickError::merge_r29_target || e == MsmPickError::rc_lanes) ? ZKMI_ERR_INVALID : ZKMI_ERR_UNSUPPORTED;
}
inline const char* msm_pick_message(MsmPickError e) {
    switch (e) {
    case MsmPickError::merge_g2: return "msm_accumulate: merge mode is implemented for G1 only";
    case MsmPickError::merge_r29_target: return "msm_accumulate: merge target holds R'-form buckets";
    case MsmPickError::r29_needs_wave: return "msm_reduce: R'-form buckets need the wave row/column sums";
    case MsmPickError::rc_lanes: return "msm_reduce: ZKMI_RC_LANES / ZKMI_RC_LANES_G2 must be 8, 16, 32 or 64";
    default: return "";
    }
}

// Block shapes that the kernels fix in their __launch_bounds__ (msm_host.hpp asserts that they agree with msm.cuh / msm29.cuh)
constexpr unsigned msm_wide_block(int limbs) { return limbs > 9 ? 128u : 256u; }      // every Fq2 kernel with LDS-parked accumulators: MsmAccumBlock<Fp2<C>>
constexpr unsigned MSM_G2S_LANES = 128;                                               // schedule lanes per 256-thread block of k_msm_accum29_g2s
// the wave row / column sums need >= 64 buckets per row and column
constexpr bool msm_wave_bits(uint32_t rbits, uint32_t cbits) { return rbits >= 6 && cbits >= 6; }

struct MsmAccumPick {
    MsmAccumKernel kernel;
    unsigned threads;               // per block
    unsigned lanes_per_block;       // grid = ceil(schedule lanes / lanes_per_block)
    bool lds;                       // the accumulators live in dynamic LDS
    bool r29_buckets;               // the finished buckets hold R'-form words
    MsmPickError error;
};
// group: 1 | 2; limbs: 9 (BN254) | 14 (BLS12-381); table29: the bases are a window table in R'-form; merge: the points are added into the buckets of
// an earlier job, which hold R'-form words iff into_r29; c: window width; compact_code: what the box asks for (zkmi_common.hpp: compact_code())
inline MsmAccumPick msm_accum_pick(int group, int limbs, bool table29, bool merge, bool into_r29, int c, int compact_code, const MsmTuning& t) {
    typedef MsmAccumKernel K;
    const bool wave_c = (c - 1) / 2 >= 6;                    // msm_wave_bits of this width: rbits = (c-1)/2 <= cbits
    if (group == 2) {
        if (merge) return {K::accum32_wide, 0, 0, false, false, MsmPickError::merge_g2};
        const unsigned T = msm_wide_block(limbs);
        if (!table29) return {K::accum32_wide, T, T, true, false, MsmPickError::none};
        // The Fq2 buckets stay in R'-form and k_msm_rowcol_wave29_g2 forms the row / column sums on the same limbs (r03 A/B, same box: BLS12-381
        // 51.1 / 50.2 against 50.3 / 50.0 proofs/s, BN254 105.9 against 105.5). On a slow-fetch box (bit 3) the sums go back to the generic 32-bit
        // kernel, whose 55 - 84 KB of code was not affected there, instead of the 320 - 750 KB of k_msm_rowcol_wave29_g2 (7.1 instead of 2.1 ms)
        const bool r29 = t.rowcol_wave && t.r29_reduce_g2 && !(compact_code & 8) && wave_c;
        // r06: one Fq2 component per lane, accumulators in registers — BN254: 168 VGPRs, 3 waves per SIMD, bit-identical buckets; BLS12-381: XYZZ in
        // 248 VGPRs without a spill instead of the packed Jacobian in LDS with 111 spilled registers (another representative of the same bucket), and
        // a hot loop of 61 KB instead of 118 KB — it fits the instruction cache, so it also takes the place of the Compact instantiation
        if (t.g2_split && !(limbs == 14 && !t.g2_split_bls)) return {K::accum29_g2s, 256, MSM_G2S_LANES, false, r29, MsmPickError::none};
        // BN254's 72 KB loop loses more to the calls (3.5 -> 7.8 ms on a healthy box) than a slow-fetch box costs it (+8 %): 14-limb curve only
        const bool compact = limbs == 14 && (compact_code & 2);
        return {compact ? K::accum29_g2_compact : K::accum29_g2, T, T, true, r29, MsmPickError::none};
    }
    if (!table29) {
        if (merge && into_r29) return {K::accum32_merge, 0, 0, false, false, MsmPickError::merge_r29_target};
        return {merge ? K::accum32_merge : K::accum32, 256, 256, false, false, MsmPickError::none};
    }
    // Threads per block. A workgroup is placed only when EVERY one of its waves finds registers: a 256-thread block needs a free slot on all four
    // SIMDs of a CU. While the Fq2 bucket reduction runs beside it on the auxiliary stream (256-register waves on two of the four SIMDs), a second
    // 14-limb accumulation block (224 registers per wave) no longer fits and the CU drops from eight to four accumulation waves (r03 trace: B1
    // 4.5 ms against 2.1 ms for the same work alone); 128-thread blocks still fill the other two SIMDs.
    const unsigned T = (t.acc29_block == 64 || t.acc29_block == 128 || t.acc29_block == 256) ? (unsigned)t.acc29_block : (limbs == 14 ? 128u : 256u);
    // the instantiation with CALLED products where the inlined loop exceeds the instruction cache (14-limb curve) and this box fetches
    // instructions slowly beyond it (field29.cuh: Compact)
    const bool compact = limbs == 14 && (compact_code & 1);
    const bool r29 = merge ? into_r29 : (t.r29_reduce && t.rowcol_wave && wave_c);
    return {compact ? (merge ? K::accum29_compact_merge : K::accum29_compact) : (merge ? K::accum29_merge : K::accum29), T, T, false, r29, MsmPickError::none};
}

struct MsmRowcolPick {
    MsmRowcolKernel kernel;
    unsigned threads;               // per block; a wave form sums threads / lanes rows or columns per block
    size_t max_blocks;              // cap on the grid of a wave form (SIZE_MAX: none)
    bool bitsums_lds;               // the plain bit sums of few arrays by k_msm_bitsums_lds instead of k_msm_bitsums
    MsmPickError error;
    unsigned lanes;                 // per sum: a block of a wave form sums threads / lanes rows or columns (wave29, wave29_compact, wave29_g2: 8, 16, 32 or 64;
                                    // wave: 64; staged: 0, its lanes per sum follow from the row length in msm_reduce)
};
constexpr bool msm_rc_lanes_ok(int v) { return v == 8 || v == 16 || v == 32 || v == 64; }
// Lanes per row / column sum of the two R'-form wave kernels where no switch forces them. n_sums: the sums of the launch, 2 * 2^cbits per bucket set
// (0: not known). Measured on one box (profiles/r07_rowcol_lanes_ab.md), BN254 Groth16 at 2^20, c = 20:
//   G1 (three bucket sets in one launch, main stream): 488 us at 64 lanes, 672 at 32, 817 at 16, 920 at 8, and the headline falls with it (112.5 -> 110.7 ->
//      108.9 -> 106.6 proofs/s). The launch has 6 144 sums for 3 072 wave slots; fewer lanes make fewer waves than the chip has SIMDs, each with a chain of
//      37 - 131 dependent additions instead of 22, and nothing else on that stream fills the idle SIMDs. G1 keeps 64, whatever the number of jobs.
//   G2 on the auxiliary stream (one bucket set, at most aux_rc_sums waves): the kernel itself gets slower too (1.40 ms at 64, 1.69 at 32, 2.24 at 16, 4.58
//      at 8) but runs underneath the G1 accumulations, which get back the issue slots it no longer takes: 16 lanes gave 114.8 / 114.8 / 114.0 proofs/s
//      against 113.5 / 112.5 / 112.5 (32: 113.4 - 114.1, 8: 112.7 - 113.0). Measured for the 9-limb curve only; alone on the main stream 64 is the fastest.
inline unsigned msm_rc_lanes_default(int group, int limbs, uint32_t rbits, uint32_t cbits, bool aux, size_t n_sums) {
    (void)rbits; (void)cbits; (void)n_sums;
    return group == 2 && aux && limbs == 9 ? 16u : 64u;
}
// all_r29: the jobs' buckets hold R'-form words; rbits / cbits: bits of the row / column index; aux: the reduction runs on the auxiliary stream;
// n_sums: row and column sums of the launch over all its jobs (0: not known) — read by the lane count alone
inline MsmRowcolPick msm_rowcol_pick(int group, int limbs, bool all_r29, uint32_t rbits, uint32_t cbits, bool aux, int compact_code, const MsmTuning& t, size_t n_sums = 0) {
    typedef MsmRowcolKernel K;
    const bool wave = t.rowcol_wave && msm_wave_bits(rbits, cbits);
    const bool bitsums_lds = group == 2 && t.rowcol_wave;
    if (all_r29 && !wave) return {K::staged, 256, SIZE_MAX, bitsums_lds, MsmPickError::r29_needs_wave, 0};
    if (!wave) return {K::staged, 256, SIZE_MAX, bitsums_lds, MsmPickError::none, 0};
    const unsigned T = group == 2 ? msm_wide_block(limbs) : 256u;
    // on the auxiliary stream at most aux_rc_sums waves are in flight (see k_msm_rowcol_wave), a quarter of the chip's CUs at two
    // 256-lane blocks per CU; the rest of the CUs stay with the main stream. The cap counts waves, however many sums a wave holds
    const size_t max_blocks = aux && t.aux_rc_sums > 0 ? (size_t)t.aux_rc_sums / (T / 64) : SIZE_MAX;
    if (!all_r29) return {K::wave, T, max_blocks, bitsums_lds, MsmPickError::none, 64};
    const int forced = group == 2 ? t.rc_lanes_g2 : t.rc_lanes;
    if (forced && !msm_rc_lanes_ok(forced)) return {group == 2 ? K::wave29_g2 : K::wave29, T, max_blocks, bitsums_lds, MsmPickError::rc_lanes, 0};
    const unsigned lanes = forced ? (unsigned)forced : msm_rc_lanes_default(group, limbs, rbits, cbits, aux, n_sums);
    if (group == 2) return {K::wave29_g2, T, max_blocks, bitsums_lds, MsmPickError::none, lanes};
    // slow-fetch box, 14-limb curve (254 KB inlined): 5.9 -> 3.0 ms there; BN254's 114 KB kernel gains nothing from the calls (measured)
    return {limbs == 14 && (compact_code & 4) ? K::wave29_compact : K::wave29, T, max_blocks, bitsums_lds, MsmPickError::none, lanes};
}

}  // namespace zkmi
