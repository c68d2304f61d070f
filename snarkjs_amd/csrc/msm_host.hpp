// snarkjs_amd/csrc/msm_host.hpp — host driver of the device Pippenger (launch sequence + final window fold).
#pragma once
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "host_field.hpp"
#include "msm.cuh"
#include "msm29.cuh"
#include <type_traits>
#include "zkmi_common.hpp"
#include "msm_select.hpp"

namespace zkmi {

static inline int ilog2_sz(size_t n) { int l = 0; while (((size_t)1 << (l + 1)) <= n) l++; return l; }

// Window width for n terms. Signed digits -> 2^(c-1) buckets per window; the table balances n·W mixed additions in
// k_msm_accum against the latency-bound bucket reduction (depth O(c)); re-tuned on MI355X.
static inline int msm_pick_c(size_t n) {
    int lg = ilog2_sz(n ? n : 1);
    if (lg < 62 && n > (((size_t)3) << lg) / 2) lg++;      // round to the nearest power of two (nVars is usually just below one)
    // (17..21 use 15: see msm_precomp_c about the fill of the top digit window)
    static const int T[] = {2, 2, 2, 3, 3, 4, 4, 5, 6, 7, 8, 9, 9, 10, 11, 11, 12, 15, 15, 15, 15, 15, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16};
    return T[lg > 31 ? 31 : lg];
}

// Host-side adapters: F = device field type; HC = host curve over the matching host field.
template <class F> struct HostOf;
template <> struct HostOf<Fp<Bn254Fq>> { typedef host::HField<4> FT; static FT make() { return host::HField<4>::from_cfg<Bn254Fq>(); } };
template <> struct HostOf<Fp2<Bn254Fq>> { typedef host::HField2<4> FT; static FT make() { return FT{host::HField<4>::from_cfg<Bn254Fq>()}; } };
template <> struct HostOf<Fp<Bls12381Fq>> { typedef host::HField<6> FT; static FT make() { return host::HField<6>::from_cfg<Bls12381Fq>(); } };
template <> struct HostOf<Fp2<Bls12381Fq>> { typedef host::HField2<6> FT; static FT make() { return FT{host::HField<6>::from_cfg<Bls12381Fq>()}; } };

// XYZZ (device words) -> host Jacobian with Z = ZZ*ZZZ:  X' = X*ZZ*ZZZ^2, Y' = Y*ZZ^3*ZZZ^2
template <class F> typename host::HCurve<typename HostOf<F>::FT>::P xyzz_to_jac(const host::HCurve<typename HostOf<F>::FT>& cv, const uint32_t* p) {
    typedef typename HostOf<F>::FT FT;
    typedef typename FT::E E;
    constexpr int FW = FieldWords<F>::value;
    const FT& Fh = cv.F;
    E X, Y, ZZ, ZZZ;
    memcpy(&X, p, 4 * FW); memcpy(&Y, p + FW, 4 * FW); memcpy(&ZZ, p + 2 * FW, 4 * FW); memcpy(&ZZZ, p + 3 * FW, 4 * FW);
    if (ZZ.is_zero()) return cv.zero();
    typename host::HCurve<FT>::P q;
    E z2 = Fh.sqr(ZZZ), zzX = Fh.mul(ZZ, z2);
    q.X = Fh.mul(X, zzX);
    q.Y = Fh.mul(Y, Fh.mul(Fh.sqr(ZZ), zzX));
    q.Z = Fh.mul(ZZ, ZZZ);
    return q;
}
// Fold the per-window device results into one Jacobian point. Per window w the device leaves (see msm.cuh, bucket
// reduction): win[(2w)*PW] = WR = sum_r r*Row_r, win[(2w+1)*PW] = WC = sum_c c*Col_c and tot[(2w)*PW] = T = sum_r Row_r;
// S_w = 2^cbits * WR + WC + T, result = sum_w 2^(c*w) * S_w (the reference also recombines windows on the host, @213360).
template <class F> void msm_fold_windows(const uint32_t* win, const uint32_t* tot, int W, int c, int cbits, uint8_t* out_jac) {
    typedef typename HostOf<F>::FT FT;
    host::HCurve<FT> cv{HostOf<F>::make()};
    constexpr int FW = FieldWords<F>::value, PW = 4 * FW;
    typename host::HCurve<FT>::P acc = cv.zero();
    for (int w = W - 1; w >= 0; w--) {
        if (!cv.is_zero(acc)) for (int k = 0; k < c; k++) acc = cv.dbl(acc);
        auto wr = xyzz_to_jac<F>(cv, win + (size_t)(2 * w) * PW);
        for (int k = 0; k < cbits && !cv.is_zero(wr); k++) wr = cv.dbl(wr);
        auto s = cv.add(cv.add(wr, xyzz_to_jac<F>(cv, win + (size_t)(2 * w + 1) * PW)), xyzz_to_jac<F>(cv, tot + (size_t)(2 * w) * PW));
        acc = cv.add(acc, s);
    }
    if (cv.is_zero(acc)) { memset(out_jac, 0, 3 * 4 * FW); return; }
    memcpy(out_jac, &acc.X, 4 * FW); memcpy(out_jac + 4 * FW, &acc.Y, 4 * FW); memcpy(out_jac + 8 * FW, &acc.Z, 4 * FW);
}

// out = a + b for two Jacobian points in the C-ABI format (host, O(1)): combines per-GPU partial MSM results.
template <class F> int point_add_host(const uint8_t* a, const uint8_t* b, uint8_t* out) {
    typedef typename HostOf<F>::FT FT;
    host::HCurve<FT> cv{HostOf<F>::make()};
    constexpr int FW = FieldWords<F>::value;
    typename host::HCurve<FT>::P p, q;
    memcpy(&p.X, a, 4 * FW); memcpy(&p.Y, a + 4 * FW, 4 * FW); memcpy(&p.Z, a + 8 * FW, 4 * FW);
    memcpy(&q.X, b, 4 * FW); memcpy(&q.Y, b + 4 * FW, 4 * FW); memcpy(&q.Z, b + 8 * FW, 4 * FW);
    auto r = cv.add(p, q);
    if (cv.is_zero(r)) { memset(out, 0, 12 * FW); return ZKMI_OK; }
    memcpy(out, &r.X, 4 * FW); memcpy(out + 4 * FW, &r.Y, 4 * FW); memcpy(out + 8 * FW, &r.Z, 4 * FW);
    return ZKMI_OK;
}
template <class F> int to_affine_host(const uint8_t* jac, uint8_t* aff) {
    typedef typename HostOf<F>::FT FT;
    host::HCurve<FT> cv{HostOf<F>::make()};
    constexpr int FW = FieldWords<F>::value;
    typename host::HCurve<FT>::P p;
    memcpy(&p.X, jac, 4 * FW); memcpy(&p.Y, jac + 4 * FW, 4 * FW); memcpy(&p.Z, jac + 8 * FW, 4 * FW);
    typename FT::E x, y;
    cv.to_affine(p, x, y);
    memcpy(aff, &x, 4 * FW); memcpy(aff + 4 * FW, &y, 4 * FW);
    return ZKMI_OK;
}

// ---- stage 1-3 (field independent, msm_sort.hip): signed-digit recoding + counting sort of all windows -----------
// The plan points into the library's named scratch buffers; it stays valid until the next msm_sort on the stream.
struct MsmPlan {
    MsmShape sh;
    int slot = 0;                     // which set of plan buffers (0/1): two plans stay alive when their MSMs are reduced in one batch
    size_t total = 0;                 // W * nb buckets
    uint32_t cap = 0;                 // lane-group granularity (msm.cuh: k_msm_assign)
    size_t lane_bound = 0, multi_bound = 0;
    uint32_t *counts = nullptr, *starts = nullptr, *sorted = nullptr;
    uint32_t *lane_g = nullptr, *lane_sub = nullptr, *meta = nullptr, *giants = nullptr;
    // which branch of the sort built the lists (host bookkeeping for zkmi_msm_sort_probe_dev; nothing on the device reads it): scalar words of the kernel
    // instantiation; radix: lb low-key bits, parts partitions, fused_cap pairs a partition may hold for k_rsort_part (0: every partition is chunked),
    // staged level-1 scatter or the direct one, and the chunk table's meta word (device: meta[0] = chunks cut by k_rsort_chunks)
    struct Path {
        int nw = 0;
        bool radix = false, staged = false;
        uint32_t lb = 0, parts = 0, fused_cap = 0;
        const uint32_t* chunk_meta = nullptr;
    } path;
};
constexpr int MSM_TB = 128, MSM_LOG_TB = 7;      // tree block: 128 lanes x 384 B (BLS12-381 G2 XYZZ) = 48 KiB of LDS
// precomp_c != 0: the bases of every MSM run over this plan are pre-computed window tables built with that c
// d_dropmask: optional bitmap over the scalars; set bits are left out of the lists (bases at infinity)
int msm_sort(const void* d_scalars, size_t n, size_t sb, MsmPlan& plan, int plan_slot = 0, int precomp_c = 0, size_t table_stride = 0, const uint32_t* d_dropmask = nullptr);

// One MSM in flight: per-window sums land in a pinned host slot; msm_fold turns them into the Jacobian result.
struct MsmJob {
    int W = 0, c = 0, cbits = 0, slot = 0;
    bool merged = false;                            // accumulated into another job's buckets (msm_accumulate `into`)
    bool r29 = false;                               // the buckets hold R'-form words (msm29.cuh): reduced by k_msm_rowcol_wave29
    int bitsums = 0;                                // h_win holds per (array, k) plain sums (k_msm_bitsums) instead of weighted sums
    uint32_t nb = 0;
    uint32_t* h_win = nullptr;                      // pinned host: 2W weighted sums then 2W totals (XYZZ)
    const uint32_t *buckets = nullptr, *counts = nullptr;   // device: this job's complete buckets (between accumulate and reduce)
    hipEvent_t acc0 = nullptr, acc1 = nullptr;      // bracket the k_msm_accum launch (bench.py roofline: live kernel time)
    // which kernels the picks chose and where msm_reduce left this job's row / column sums (host bookkeeping for zkmi_msm_stage_probe_dev, as
    // MsmPlan::Path is for the sort probe; nothing on the device reads it): MsmAccumKernel / MsmRowcolKernel as integers, -1 before the stage has run
    int accum_kernel = -1, rowcol_kernel = -1;
    const uint32_t* rowcol = nullptr;               // device: 2 W 2^cbits XYZZ points, ((w * 2 + kind) << cbits) + i; valid until the next msm_reduce on the stream
};
constexpr int MSM_JOB_SLOTS = 8;
constexpr size_t MSM_JOB_SLOT_BYTES = 512 * 1024;
int msm_job_slot(int slot, MsmJob& job);

// Raises a kernel's limit of dynamic LDS to `bytes`, once per kernel and process (every caller of one kernel passes the same size).
template <auto Kernel> int lds_opt_in(size_t bytes) {
    static bool opted = false;
    if (!opted) {
        ZK_HIP(hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        opted = true;
    }
    return ZKMI_OK;
}
static inline int msm_pick_fail(MsmPickError e) { return fail(msm_pick_code(e), msm_pick_message(e)); }
// zkmi_msm_rowcol_lanes (include/zkmi_diag.h): lanes per row / column sum of the last msm_reduce of G1 | G2 (host bookkeeping like MsmJob::rowcol_kernel, which
// stays as it is: the probe's info record has no room for it); 0: none yet, or the staged sums
inline int g_msm_rowcol_lanes[2] = {0, 0};

// ---- stage 4: bucket accumulation for one base table over an existing plan ---------------------------------------------
// skip: the scalar with index i pairs with base (i - skip); indices < skip are ignored. This lets several MSMs share
// one digit sort (Groth16: A, B1, B2 over the witness and C over witness[nPublic+1:], src/groth16_prove.js:85-97).
// Leaves the complete buckets of this MSM in the bucket buffer of job.slot; msm_reduce finishes the job.
// into (optional): an already accumulated job of the same shape; this MSM's points are added into ITS buckets (the two results are
// only needed as a sum) and `job` is marked merged: msm_reduce skips it and msm_fold returns the point at infinity for it.
template <class F> int msm_accumulate(const void* d_bases, const MsmPlan& pl, uint32_t skip, MsmJob& job, const uint32_t* d_infmask = nullptr, MsmJob* into = nullptr) {
    constexpr int FW = FieldWords<F>::value, PW = 4 * FW;
    constexpr bool WIDE = FW > 12;                                     // G2
    typedef typename F::Cfg C;
    constexpr int NL = Lim29<C>::NL;
    static_assert(!WIDE || (Accum29G2<C>::T == msm_wide_block(NL) && MsmAccumBlock<F>::value == msm_wide_block(NL)), "msm_select.hpp: block of the Fq2 kernels");
    static_assert(G2S_SLOTS == MSM_G2S_LANES, "msm_select.hpp: lanes per block of k_msm_accum29_g2s");
    Ctx& cx = ctx();
    const MsmShape& sh = pl.sh;
    const size_t total = pl.total;
    hipStream_t st = cx.stream;
    const std::string sfx = "." + std::to_string(job.slot);
    // base arrays registered in the R'-form of field29.cuh (window tables of resident bases; the library's own upload of a plain zkmi_msm
    // call): the hot loop on unsaturated limbs (9 x 29 bits BN254, 14 x 28 bits BLS12-381)
    auto r29 = cx.r29_tables.find(d_bases);
    const bool table29 = r29 != cx.r29_tables.end();
    const int box = table29 && (WIDE || NL > 9) ? compact_code() : 0;  // the box is probed on first use, and only where a rule of the pick reads it
    const MsmAccumPick pick = msm_accum_pick(WIDE ? 2 : 1, NL, table29, into != nullptr, into && into->r29, sh.c, box, msm_tuning());
    if (pick.error == MsmPickError::merge_g2) return msm_pick_fail(pick.error);      // refused before the target is looked at
    uint32_t *buckets, *lane_partials, *block_partials;
    const uint32_t* prev_counts = nullptr;
    if (into) {
        if (into->W != sh.W || into->c != sh.c || into->nb != sh.nb || !into->buckets) return fail(ZKMI_ERR_INVALID, "msm_accumulate: merge target of a different shape");
        buckets = const_cast<uint32_t*>(into->buckets);
        prev_counts = into->counts;
    } else ZK_TRY(ws_get("msm.buckets" + sfx, total * PW * 4, (void**)&buckets));
    if (pick.error != MsmPickError::none) return msm_pick_fail(pick.error);          // a target of the right shape in the wrong form
    ZK_TRY(ws_get("msm.lane_partials", std::max<size_t>(pl.multi_bound, 1) * PW * 4, (void**)&lane_partials));
    const size_t tree_blocks = pl.multi_bound / MSM_TB + 1;
    ZK_TRY(ws_get("msm.block_partials", tree_blocks * PW * 4, (void**)&block_partials));
    const size_t tree_lds = (size_t)MSM_TB * PW * 4;
    ZK_TRY((lds_opt_in<k_msm_tree<F, MSM_TB>>(tree_lds)));
    ZK_TRY((lds_opt_in<k_msm_giant<F, MSM_TB>>(tree_lds)));
    const dim3 grid((unsigned)((pl.lane_bound + pick.lanes_per_block - 1) / pick.lanes_per_block)), block(pick.threads);
    const uint32_t* mask = d_infmask ? d_infmask : (table29 ? r29->second : nullptr);
    const int r29_flag = (int)pick.r29_buckets;
    // one argument list per kernel signature; grid and block come from the pick
    auto launch29 = [&](auto kernel) {                                 // G1 on unsaturated limbs
        hipLaunchKernelGGL(kernel, grid, block, 0, st, (const uint32_t*)d_bases, mask, sh, skip, pl.cap, pl.counts, pl.starts, pl.sorted, pl.lane_g, pl.lane_sub, pl.meta, buckets,
                           lane_partials, prev_counts, r29_flag);
    };
    auto launch29_g2 = [&](auto kernel, size_t lds) {                  // G2 on unsaturated limbs: no merge mode
        hipLaunchKernelGGL(kernel, grid, block, lds, st, (const uint32_t*)d_bases, mask, sh, skip, pl.cap, pl.counts, pl.starts, pl.sorted, pl.lane_g, pl.lane_sub, pl.meta, buckets,
                           lane_partials, r29_flag);
    };
    auto launch32 = [&](auto kernel, size_t lds) {                     // saturated 32-bit words, R-form buckets
        hipLaunchKernelGGL(kernel, grid, block, lds, st, (const uint32_t*)d_bases, mask, sh, skip, pl.cap, pl.counts, pl.starts, pl.sorted, pl.lane_g, pl.lane_sub, pl.meta, buckets,
                           lane_partials, prev_counts);
    };
    if (job.acc0) ZK_HIP(hipEventRecord(job.acc0, st));
    typedef MsmAccumKernel K;
    switch (pick.kernel) {                                             // a case outside its `if constexpr` is one the pick never gives for this F
    case K::accum29: if constexpr (!WIDE) launch29(k_msm_accum29<C, false>); break;
    case K::accum29_merge: if constexpr (!WIDE) launch29(k_msm_accum29<C, true>); break;
    case K::accum29_compact: if constexpr (!WIDE && NL > 9) launch29(k_msm_accum29<Compact<C>, false>); break;
    case K::accum29_compact_merge: if constexpr (!WIDE && NL > 9) launch29(k_msm_accum29<Compact<C>, true>); break;
    case K::accum29_g2s: if constexpr (WIDE) launch29_g2(k_msm_accum29_g2s<C>, 0); break;
    case K::accum29_g2:
    case K::accum29_g2_compact:
        if constexpr (WIDE) {
            constexpr size_t lds29 = Accum29G2<C>::lds_bytes;          // 4 coordinates x 2 components per lane
            ZK_TRY(lds_opt_in<k_msm_accum29_g2<C>>(lds29));
            if constexpr (NL > 9) {
                ZK_TRY(lds_opt_in<k_msm_accum29_g2<Compact<C>>>(lds29));
                if (pick.kernel == K::accum29_g2_compact) { launch29_g2(k_msm_accum29_g2<Compact<C>>, lds29); break; }
            }
            launch29_g2(k_msm_accum29_g2<C>, lds29);
        }
        break;
    case K::accum32: if constexpr (!WIDE) launch32(k_msm_accum<F, false, false>, 0); break;
    case K::accum32_merge: if constexpr (!WIDE) launch32(k_msm_accum<F, false, true>, 0); break;
    case K::accum32_wide:
        if constexpr (WIDE) {
            const size_t acc_lds = (size_t)PW * pick.threads * 4;      // XYZZ accumulators live in LDS
            ZK_TRY((lds_opt_in<k_msm_accum<F, true, false>>(acc_lds)));
            launch32(k_msm_accum<F, true, false>, acc_lds);
        }
        break;
    }
    if (job.acc1) ZK_HIP(hipEventRecord(job.acc1, st));
    if (cx.msm_stats && cx.d_addcount && job.slot < MSM_JOB_SLOTS) {           // outside the bracketed launch
        const int ci = cx.pipe * MSM_JOB_SLOTS + job.slot;
        ZK_HIP(hipMemsetAsync(cx.d_addcount + ci, 0, 8, st));
        hipLaunchKernelGGL(k_msm_count_adds, dim3(1024), dim3(256), 0, st, pl.sorted, pl.counts, pl.starts, (uint32_t)total, skip, mask, cx.d_addcount + ci);
        ZK_HIP(hipMemcpyAsync(cx.h_addcount + ci, cx.d_addcount + ci, 8, hipMemcpyDeviceToHost, st));
    }
    hipLaunchKernelGGL((k_msm_tree<F, MSM_TB>), dim3((unsigned)std::min<size_t>(tree_blocks, 512)), dim3(MSM_TB), tree_lds, st, lane_partials, pl.lane_g, pl.counts, pl.cap, pl.meta, buckets,
                       block_partials, r29_flag);
    hipLaunchKernelGGL((k_msm_giant<F, MSM_TB>), dim3((unsigned)std::min<size_t>(tree_blocks, 256)), dim3(MSM_TB), tree_lds, st, pl.giants, pl.meta, block_partials, buckets, r29_flag);
    job.W = sh.W; job.c = sh.c; job.nb = sh.nb; job.buckets = buckets; job.counts = pl.counts;
    job.merged = into != nullptr;
    job.r29 = pick.r29_buckets;
    job.accum_kernel = (int)pick.kernel;
    if (into) {
        uint32_t* cmb;
        ZK_TRY(ws_get("msm.cmbcounts." + std::to_string(into->slot), total * 4, (void**)&cmb));
        hipLaunchKernelGGL(k_msm_counts_add, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, prev_counts, pl.counts, (uint32_t)total, cmb);
        into->counts = cmb;
    }
    ZK_HIP(hipGetLastError());
    return ZKMI_OK;
}

// ---- stage 5: bucket reduction of up to MSM_MAX_BATCH accumulated jobs of the same shape, in one set of launches ------
// aux: run on the library's auxiliary stream with its own scratch buffers (a latency-bound reduction can then overlap the
// throughput-bound accumulations of other MSMs); the caller orders the streams with events.
template <class F> int msm_reduce(MsmJob* const* jobs, int njobs, bool aux = false) {
    constexpr int FW = FieldWords<F>::value, PW = 4 * FW;
    Ctx& cx = ctx();
    hipStream_t st = aux ? cx.aux_stream : cx.stream;
    const std::string ax = aux ? ".aux" : "";
    if (njobs < 1 || njobs > MSM_MAX_BATCH) return fail(ZKMI_ERR_INVALID, "msm_reduce: bad batch size");
    const int W = jobs[0]->W, c = jobs[0]->c;
    const uint32_t nb = jobs[0]->nb;
    MsmReduceBatch rb;
    rb.njobs = njobs;
    for (int i = 0; i < njobs; i++) {
        if (jobs[i]->W != W || jobs[i]->c != c) return fail(ZKMI_ERR_INVALID, "msm_reduce: jobs of different shape");
        rb.buckets[i] = jobs[i]->buckets; rb.counts[i] = jobs[i]->counts;
    }
    const uint32_t rbits = (uint32_t)(c - 1) / 2, cbits = (uint32_t)(c - 1) - rbits, C = 1u << cbits;
    const size_t VW = (size_t)njobs * W * 2;                           // arrays of C points: (job, window, row|col)
    constexpr int M = (PW * 4 * 2 * 256 <= 128 * 1024) ? 256 : 128;    // k_msm_wsum: 2 LDS arrays of M points
    const uint32_t m2 = (C + M - 1) / M;
    uint32_t *rc, *a0, *r0, *a1, *r1;
    ZK_TRY(ws_get("msm.rowcol" + ax, VW * C * PW * 4, (void**)&rc));
    ZK_TRY(ws_get("msm.redA0" + ax, std::max<size_t>(VW * m2, VW * (cbits + 1)) * PW * 4, (void**)&a0));
    ZK_TRY(ws_get("msm.redR0" + ax, VW * m2 * PW * 4, (void**)&r0));
    ZK_TRY(ws_get("msm.redA1" + ax, VW * PW * 4, (void**)&a1));
    ZK_TRY(ws_get("msm.redR1" + ax, VW * PW * 4, (void**)&r1));
    const size_t n_out = VW * C;
    constexpr bool WIDE_R = FW > 12;
    typedef typename F::Cfg Cfg;
    constexpr int NL = Lim29<Cfg>::NL;
    static_assert(MsmRcBlock<F>::value == (WIDE_R ? msm_wide_block(NL) : 256u) && (!WIDE_R || Reduce29G2<Cfg>::T == msm_wide_block(NL)), "msm_select.hpp: block of the wave sums");
    bool all_r29 = true;                                     // R'-form buckets and the row / column sums on the same limbs
    for (int i = 0; i < njobs; i++) all_r29 = all_r29 && jobs[i]->r29;
    for (int i = 0; i < njobs; i++) if (jobs[i]->r29 != jobs[0]->r29) return fail(ZKMI_ERR_INVALID, "msm_reduce: jobs with different bucket formats");
    const int box = !WIDE_R && NL > 9 && all_r29 ? compact_code() : 0;      // as in msm_accumulate: only where a rule reads it
    const MsmRowcolPick rp = msm_rowcol_pick(WIDE_R ? 2 : 1, NL, all_r29, rbits, cbits, aux, box, msm_tuning(), n_out);
    if (rp.error != MsmPickError::none) return msm_pick_fail(rp.error);
    const size_t per_block = rp.threads / (rp.lanes ? rp.lanes : 64u), rc_blocks = std::min((n_out + per_block - 1) / per_block, rp.max_blocks);
    auto launch_wave = [&](auto kernel, size_t lds) {         // rp.lanes lanes per sum with the fold inside the launch
        hipLaunchKernelGGL(kernel, dim3((unsigned)rc_blocks), dim3(rp.threads), lds, st, rb, (uint32_t)W, nb, rbits, cbits, rc);
    };
    // the instantiation for the picked lanes per sum: f is handed the lane count as a compile-time constant
    auto with_lanes = [&](auto&& f) {
        switch (rp.lanes) {
        case 8: return f(std::integral_constant<int, 8>());
        case 16: return f(std::integral_constant<int, 16>());
        case 32: return f(std::integral_constant<int, 32>());
        default: return f(std::integral_constant<int, 64>());
        }
    };
    switch (rp.kernel) {
    case MsmRowcolKernel::wave29:
    case MsmRowcolKernel::wave29_compact:
        if constexpr (!WIDE_R) {
            constexpr size_t lds29 = (size_t)256 * 4 * NL * 4;
            ZK_TRY(with_lanes([&](auto lps) {
                constexpr int LPS = decltype(lps)::value;
                if constexpr (NL > 9) {
                    if (rp.kernel == MsmRowcolKernel::wave29_compact) {
                        ZK_TRY((lds_opt_in<k_msm_rowcol_wave29<Compact<Cfg>, LPS>>(lds29)));
                        launch_wave(k_msm_rowcol_wave29<Compact<Cfg>, LPS>, lds29);
                        return (int)ZKMI_OK;
                    }
                }
                ZK_TRY((lds_opt_in<k_msm_rowcol_wave29<Cfg, LPS>>(lds29)));
                launch_wave(k_msm_rowcol_wave29<Cfg, LPS>, lds29);
                return (int)ZKMI_OK;
            }));
        }
        break;
    case MsmRowcolKernel::wave29_g2:
        if constexpr (WIDE_R) {
            ZK_TRY(with_lanes([&](auto lps) {
                constexpr int LPS = decltype(lps)::value;
                ZK_TRY((lds_opt_in<k_msm_rowcol_wave29_g2<Cfg, LPS>>(Reduce29G2<Cfg>::lds_bytes)));
                launch_wave(k_msm_rowcol_wave29_g2<Cfg, LPS>, Reduce29G2<Cfg>::lds_bytes);
                return (int)ZKMI_OK;
            }));
        }
        break;
    case MsmRowcolKernel::wave: {
        const size_t lds_rc = (size_t)rp.threads * PW * 4;
        ZK_TRY(lds_opt_in<k_msm_rowcol_wave<F>>(lds_rc));
        launch_wave(k_msm_rowcol_wave<F>, lds_rc);
        break;
    }
    case MsmRowcolKernel::staged: {
        // Row/Col sums in stages: L lanes per sum (~16 additions each), then folds of 8 partials at a time
        // (Fq2 additions are ~50 us of latency each and the total work is small: spread wider and fold 4 at a time)
        const uint32_t seq = WIDE_R ? 4 : 16, maxL = WIDE_R ? 256 : 64, foldK = WIDE_R ? 4 : 8;
        uint32_t L = 1;
        while (L < maxL && (C / L) > seq) L <<= 1;
        uint32_t *p0, *p1;
        ZK_TRY(ws_get("msm.rcpart0" + ax, n_out * L * PW * 4, (void**)&p0));
        ZK_TRY(ws_get("msm.rcpart1" + ax, std::max<size_t>(n_out * L / 4, 1) * PW * 4, (void**)&p1));
        uint32_t* dst = L == 1 ? rc : p0;
        hipLaunchKernelGGL((k_msm_rowcol<F>), dim3((unsigned)((n_out * L + 255) / 256)), dim3(256), 0, st, rb, (uint32_t)W, nb, rbits, cbits, L, dst);
        uint32_t parts = L;
        const uint32_t* src = dst;
        while (parts > 1) {
            const uint32_t K = std::min<uint32_t>(parts, foldK);
            parts /= K;
            uint32_t* d2 = parts == 1 ? rc : (src == p0 ? p1 : p0);
            hipLaunchKernelGGL((k_msm_fold<F>), dim3((unsigned)((n_out * parts + 255) / 256)), dim3(256), 0, st, src, d2, n_out * parts, K);
            src = d2;
        }
        break;
    }
    }
    const bool bitsums = VW * (cbits + 1) <= 256;            // few arrays (pre-computed tables): plain sums only, host does the weighting
    const uint32_t* resA = nullptr;
    const uint32_t* resR = nullptr;
    size_t perA = 0;                                         // words per job in resA
    if (bitsums) {
        const dim3 bgrid((unsigned)(VW * (cbits + 1)));
        if (rp.bitsums_lds) {
            if constexpr (WIDE_R) {                          // G2 only
                constexpr int TB = MsmAccumBlock<F>::value;
                ZK_TRY(lds_opt_in<k_msm_bitsums_lds<F>>((size_t)TB * PW * 4));
                hipLaunchKernelGGL((k_msm_bitsums_lds<F>), bgrid, dim3(TB), (size_t)TB * PW * 4, st, rc, C, cbits, a0);
            }
        } else {
            constexpr int MB = (PW * 4 * 256 <= 64 * 1024) ? 256 : 128;
            ZK_TRY((lds_opt_in<k_msm_bitsums<F, MB>>((size_t)MB * PW * 4)));
            hipLaunchKernelGGL((k_msm_bitsums<F, MB>), bgrid, dim3(MB), (size_t)MB * PW * 4, st, rc, C, cbits, a0);
        }
        resA = a0;
        perA = (size_t)2 * W * (cbits + 1) * PW;
    } else {
        uint32_t m = C;
        int log_scale = 0;
        const uint32_t *inA = nullptr, *inR = rc;
        uint32_t *outA = a0, *outR = r0;
        const size_t lds_ws = (size_t)2 * M * PW * 4;
        ZK_TRY((lds_opt_in<k_msm_wsum<F, M>>(lds_ws)));
        for (;;) {
            const uint32_t blocks = (m + M - 1) / M;
            hipLaunchKernelGGL((k_msm_wsum<F, M>), dim3((unsigned)(VW * blocks)), dim3(M), lds_ws, st, inA, inR, m, blocks, log_scale, outA, outR);
            inA = outA; inR = outR;
            if (blocks == 1) break;
            outA = (outA == a0) ? a1 : a0; outR = (outR == r0) ? r1 : r0;
            m = blocks;
            log_scale += ilog2_sz(M);
        }
        resA = inA; resR = inR;
        perA = (size_t)2 * W * PW;
    }
    g_msm_rowcol_lanes[WIDE_R ? 1 : 0] = (int)rp.lanes;
    for (int i = 0; i < njobs; i++) {
        MsmJob& job = *jobs[i];
        job.cbits = (int)cbits;
        job.bitsums = bitsums ? 1 : 0;
        job.rowcol_kernel = (int)rp.kernel;
        job.rowcol = rc + (size_t)i * 2 * W * C * PW;
        if (perA * 4 * 2 > MSM_JOB_SLOT_BYTES) return fail(ZKMI_ERR_UNSUPPORTED, "msm: too many windows");
        ZK_HIP(hipMemcpyAsync(job.h_win, resA + (size_t)i * perA, perA * 4, hipMemcpyDeviceToHost, st));
        if (!bitsums) ZK_HIP(hipMemcpyAsync(job.h_win + perA, resR + (size_t)i * perA, perA * 4, hipMemcpyDeviceToHost, st));
    }
    ZK_HIP(hipGetLastError());
    return ZKMI_OK;
}
// after the stream has been synchronised
template <class F> void msm_fold(const MsmJob& job, uint8_t* out_jac) {
    constexpr int PW = 4 * FieldWords<F>::value;
    if (job.merged) { memset(out_jac, 0, 3 * PW); return; }              // its points are inside the merge target's result
    if (!job.bitsums) { msm_fold_windows<F>(job.h_win, job.h_win + (size_t)2 * job.W * PW, job.W, job.c, job.cbits, out_jac); return; }
    // plain bit sums -> weighted sums by Horner on the host, laid out as msm_fold_windows expects
    typedef typename HostOf<F>::FT FT;
    host::HCurve<FT> cv{HostOf<F>::make()};
    const int nb1 = job.cbits + 1;
    std::vector<uint32_t> win((size_t)2 * job.W * PW), tot((size_t)2 * job.W * PW);
    auto put = [&](uint32_t* dst, const typename host::HCurve<FT>::P& p) {      // Jacobian -> XYZZ words (ZZ = Z^2, ZZZ = Z^3)
        constexpr int FW = FieldWords<F>::value;
        if (cv.is_zero(p)) { memset(dst, 0, PW * 4); return; }
        auto z2 = cv.F.sqr(p.Z), z3 = cv.F.mul(z2, p.Z);
        memcpy(dst, &p.X, 4 * FW); memcpy(dst + FW, &p.Y, 4 * FW); memcpy(dst + 2 * FW, &z2, 4 * FW); memcpy(dst + 3 * FW, &z3, 4 * FW);
    };
    for (int a = 0; a < 2 * job.W; a++) {
        const uint32_t* src = job.h_win + (size_t)a * nb1 * PW;
        auto acc = cv.zero();
        for (int k = job.cbits - 1; k >= 0; k--) { if (!cv.is_zero(acc)) acc = cv.dbl(acc); acc = cv.add(acc, xyzz_to_jac<F>(cv, src + (size_t)k * PW)); }
        put(win.data() + (size_t)a * PW, acc);
        memcpy(tot.data() + (size_t)a * PW, src + (size_t)job.cbits * PW, PW * 4);
    }
    msm_fold_windows<F>(win.data(), tot.data(), job.W, job.c, job.cbits, out_jac);
}

// ---- zkmi_msm_stage_probe_dev (include/zkmi_diag.h): the back half of ONE MSM looked at from outside ------------------------------------------
// While a sink is set (by the probe alone, for the length of its call), msm_run and msm_run_table hand over what the job they have just finished
// left on the device: finished buckets and row / column sums as affine points. A product call finds the pointer null and does nothing more.
struct MsmStageSink {
    uint8_t *buckets = nullptr, *rowcol = nullptr;  // host arrays of the caller (may be null), with room for this many points
    size_t buckets_cap = 0, rowcol_cap = 0;
    zkmi_msm_stage_info info = {};
    bool ran = false;                               // info has been written
};
MsmStageSink*& msm_stage_sink();                    // msm_sort.hip

// n XYZZ points (device words as the kernels store them, R-form or R'-form: x = X / ZZ and y = Y / ZZZ do not see a common factor of the four
// coordinates) -> affine points in the reference's R-form, all-zero for the point at infinity; live (optional): a zero word marks a point that
// was never written. One inversion in all (Montgomery's trick).
template <class F> void xyzz_words_to_affine(const uint32_t* src, const uint32_t* live, size_t n, uint8_t* dst) {
    typedef typename HostOf<F>::FT FT;
    typedef typename FT::E E;
    constexpr int FW = FieldWords<F>::value, PW = 4 * FW;
    const FT Fh = HostOf<F>::make();
    auto coord = [&](size_t i, int k) { E v; memcpy(&v, src + i * PW + (size_t)k * FW, 4 * FW); return v; };
    std::vector<E> pre(n);                          // pre[i] = product of ZZ ZZZ over the finite points before i
    std::vector<uint8_t> fin(n);
    E run = Fh.One();
    for (size_t i = 0; i < n; i++) {
        pre[i] = run;
        fin[i] = (!live || live[i]) && !coord(i, 2).is_zero();
        if (fin[i]) run = Fh.mul(run, Fh.mul(coord(i, 2), coord(i, 3)));
    }
    E inv = Fh.inv(run);
    for (size_t i = n; i-- > 0;) {
        uint8_t* o = dst + i * 2 * 4 * FW;
        if (!fin[i]) { memset(o, 0, 2 * 4 * FW); continue; }
        const E zz = coord(i, 2), zzz = coord(i, 3), both = Fh.mul(inv, pre[i]);      // 1 / (ZZ ZZZ) of this point
        inv = Fh.mul(inv, Fh.mul(zz, zzz));
        const E x = Fh.mul(coord(i, 0), Fh.mul(both, zzz)), y = Fh.mul(coord(i, 1), Fh.mul(both, zz));
        memcpy(o, &x, 4 * FW); memcpy(o + 4 * FW, &y, 4 * FW);
    }
}
// after the stream has been synchronised and the job folded
template <class F> int msm_stage_collect(MsmStageSink& sk, const MsmPlan& pl, const MsmJob& job) {
    constexpr int PW = 4 * FieldWords<F>::value;
    uint32_t m[3] = {0, 0, 0};
    ZK_HIP(hipMemcpy(m, pl.meta, sizeof m, hipMemcpyDeviceToHost));
    zkmi_msm_stage_info& r = sk.info;
    r.c = (uint32_t)job.c; r.W = (uint32_t)job.W; r.nb = job.nb; r.cbits = (uint32_t)job.cbits; r.rbits = (uint32_t)(job.c - 1 - job.cbits);
    r.accum_kernel = (uint32_t)job.accum_kernel; r.rowcol_kernel = (uint32_t)job.rowcol_kernel;
    r.r29_buckets = job.r29; r.bitsums = (uint32_t)job.bitsums;
    r.cap = pl.cap; r.lanes = m[0]; r.multi_lanes = m[1]; r.giants = m[2];
    sk.ran = true;
    const size_t total = (size_t)job.W * job.nb, n_rc = ((size_t)2 * job.W) << job.cbits;
    if (total != pl.total || !job.buckets || !job.counts || !job.rowcol) return fail(ZKMI_ERR_INVALID, "msm_stage_probe: the job did not pass through every stage");
    if ((sk.buckets && sk.buckets_cap < total) || (sk.rowcol && sk.rowcol_cap < n_rc)) return fail(ZKMI_ERR_INVALID, "msm_stage_probe: an output array is too small (sizes are in *info)");
    if (sk.buckets) {
        std::vector<uint32_t> w(total * PW), live(total);
        ZK_HIP(hipMemcpy(live.data(), job.counts, total * 4, hipMemcpyDeviceToHost));
        ZK_HIP(hipMemcpy(w.data(), job.buckets, total * PW * 4, hipMemcpyDeviceToHost));
        xyzz_words_to_affine<F>(w.data(), live.data(), total, sk.buckets);
    }
    if (sk.rowcol) {
        std::vector<uint32_t> w(n_rc * PW);
        ZK_HIP(hipMemcpy(w.data(), job.rowcol, n_rc * PW * 4, hipMemcpyDeviceToHost));
        xyzz_words_to_affine<F>(w.data(), nullptr, n_rc, sk.rowcol);
    }
    return ZKMI_OK;
}

// Full device MSM: bases (affine, device), scalars (plain integers, device) -> Jacobian point on the host.
template <class F> int msm_run(const void* d_bases, const void* d_scalars, size_t n, size_t sb, uint8_t* out_jac) {
    constexpr int FW = FieldWords<F>::value;
    Ctx& cx = ctx();
    if (n == 0) { memset(out_jac, 0, 3 * 4 * FW); return ZKMI_OK; }
    hipStream_t st = cx.stream;
    MsmPlan pl;
    MsmJob job;
    ZK_TRY(slot_idle_or_fail("msm"));
    ZK_TRY(msm_job_slot(0, job));
    if (!cx.ev0_held) ZK_HIP(hipEventRecord(cx.ev0, st));
    ZK_TRY(msm_sort(d_scalars, n, sb, pl));
    ZK_TRY(msm_accumulate<F>(d_bases, pl, 0, job));
    MsmJob* jp = &job;
    ZK_TRY(msm_reduce<F>(&jp, 1));
    ZK_HIP(hipEventRecord(cx.ev1, st));
    ZK_HIP(hipStreamSynchronize(st));
    float ms = 0;
    if (hipEventElapsedTime(&ms, cx.ev0, cx.ev1) == hipSuccess) cx.last_ms = ms;
    msm_fold<F>(job, out_jac);
    if (MsmStageSink* sk = msm_stage_sink()) return msm_stage_collect<F>(*sk, pl, job);
    return ZKMI_OK;
}

// Window width and digit count of a pre-computed table for n resident bases and sb-byte scalars
static inline int msm_precomp_c(size_t n) {
    int lg = ilog2_sz(n ? n : 1);
    if (lg < 62 && n > (((size_t)3) << lg) / 2) lg++;
    int c = std::max(8, std::min(21, lg));
    // 254/255-bit scalars: keep the top digit window well filled (a 2..7-bit top window funnels millions of scalars into a
    // handful of buckets and serialises the sort's atomics): for large n snap to c in {15, 16, 17, 20}
    if (lg >= 14) { static const int snap[] = {15, 15, 16, 17, 17, 20, 20, 20}; c = snap[std::min(std::max(c, 14), 21) - 14]; }
    return c;
}
static inline int msm_digits(size_t sb, int c) { return (int)((8 * sb + 1 + c - 1) / c); }
// d_table: Wd * n affine points (device). Built once per resident base set.
template <class F> int msm_precompute(const void* d_bases, size_t n, int c, int Wd, void* d_table) {
    Ctx& cx = ctx();
    hipLaunchKernelGGL((k_msm_precompute<F>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, cx.stream, (const uint32_t*)d_bases, (uint32_t)n, c, Wd, (uint32_t*)d_table);
    ZK_HIP(hipGetLastError());
    return ZKMI_OK;
}
int msm_precompute_dispatch(int curve, int group, const void* d_bases, size_t n, int c, int Wd, void* d_table);
template <class F> int msm_infmask(const void* d_points, size_t n, uint32_t* d_mask) {
    Ctx& cx = ctx();
    ZK_HIP(hipMemsetAsync(d_mask, 0, ((n + 31) / 32) * 4, cx.stream));
    if (n) hipLaunchKernelGGL((k_msm_infmask<F>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, cx.stream, (const uint32_t*)d_points, n, d_mask);
    ZK_HIP(hipGetLastError());
    return ZKMI_OK;
}
// MSM of the first k scalars against a pre-computed table (stride points per row, window width c)
template <class F> int msm_run_table(const void* d_table, size_t stride, int c, const void* d_scalars, size_t k, size_t sb, uint8_t* out_jac);
int msm_table_dispatch(int curve, int group, const void* d_table, size_t stride, int c, const void* d_scalars, size_t k, size_t sb, uint8_t* out_jac);
// Several MSMs against the same table (independent scalar vectors): one sort + accumulation each, ONE batched bucket reduction
int msm_table_multi_dispatch(int curve, int group, const void* d_table, size_t stride, int c, const void* const* d_scalars, const size_t* ks, int count, size_t sb,
                             uint8_t* out_jacs);

// non-template entry points (msm_bn254.hip / msm_bls12381.hip) for callers that must not instantiate the kernels again
int msm_accumulate_dispatch(int curve, int group, const void* d_bases, const MsmPlan& pl, uint32_t skip, MsmJob& job, const uint32_t* d_infmask = nullptr, MsmJob* into = nullptr);
// d_mask: ceil(n/32) words, zeroed by the callee; bit i = point i is the point at infinity
int msm_infmask_dispatch(int curve, int group, const void* d_points, size_t n, uint32_t* d_mask);
int msm_reduce_dispatch(int curve, int group, MsmJob* const* jobs, int njobs, bool aux = false);

int msm_fold_dispatch(int curve, int group, const MsmJob& job, uint8_t* out_jac);

template <class F> int msm_run_table(const void* d_table, size_t stride, int c, const void* d_scalars, size_t k, size_t sb, uint8_t* out_jac) {
    constexpr int FW = FieldWords<F>::value;
    Ctx& cx = ctx();
    if (k == 0) { memset(out_jac, 0, 3 * 4 * FW); return ZKMI_OK; }
    hipStream_t st = cx.stream;
    MsmPlan pl;
    MsmJob job;
    ZK_TRY(slot_idle_or_fail("msm_table"));
    ZK_TRY(msm_job_slot(0, job));
    ZK_HIP(hipEventRecord(cx.ev0, st));
    ZK_TRY(msm_sort(d_scalars, k, sb, pl, 0, c, stride));
    ZK_TRY(msm_accumulate<F>(d_table, pl, 0, job));
    MsmJob* jp = &job;
    ZK_TRY(msm_reduce<F>(&jp, 1));
    ZK_HIP(hipEventRecord(cx.ev1, st));
    ZK_HIP(hipStreamSynchronize(st));
    float ms = 0;
    if (hipEventElapsedTime(&ms, cx.ev0, cx.ev1) == hipSuccess) cx.last_ms = ms;
    msm_fold<F>(job, out_jac);
    if (MsmStageSink* sk = msm_stage_sink()) return msm_stage_collect<F>(*sk, pl, job);
    return ZKMI_OK;
}

// The MSMs of one zkmi_msm_table_multi call that have been enqueued and not yet collected, per pipeline slot (r06: enqueue / collect split, so that a
// host that drives two proofs from one thread — plonk.py prove_many, js proveMany — can put the accumulations of proof B on the device underneath the
// latency-bound bucket reduction of proof A instead of waiting inside A's call)
struct MsmMultiPending {
    bool live = false;
    int count = 0, fw = 0;
    size_t ks[MSM_MAX_BATCH] = {};
    MsmJob job[MSM_MAX_BATCH];
};
MsmMultiPending& msm_multi_pending(int pipe);              // msm_sort.hip

template <class F> int msm_run_table_multi_enqueue(const void* d_table, size_t stride, int c, const void* const* d_scalars, const size_t* ks, int count, size_t sb) {
    constexpr int FW = FieldWords<F>::value;
    Ctx& cx = ctx();
    if (count < 1 || count > MSM_MAX_BATCH) return fail(ZKMI_ERR_INVALID, "msm_table_multi: 1..4 MSMs per call");
    MsmMultiPending& P = msm_multi_pending(cx.pipe);
    hipStream_t st = cx.stream;
    ZK_TRY(slot_idle_or_fail("msm_table_multi", false));              // a Groth16 proof in flight; this slot's own abandoned call is dropped below instead
    if (P.live) {                                                      // a call that was enqueued and never collected (its proof was abandoned after an error): drop it
        ZK_HIP(hipStreamSynchronize(st));
        P.live = false;
    }
    MsmPlan pl[MSM_MAX_BATCH];
    MsmJob* job = P.job;
    MsmJob* jp[MSM_MAX_BATCH];
    int live = 0;
    ZK_HIP(hipEventRecord(cx.ev0, st));
    // The digit sorts are memory-bound, the accumulations ALU-bound: with more than one MSM in the call the sorts go to the
    // auxiliary stream, so that sort i+1 runs underneath accumulation i (MsmTuning::multi_overlap off keeps one stream).
    int n_live = 0;
    for (int i = 0; i < count; i++) n_live += ks[i] != 0;
    const bool ov = msm_tuning().multi_overlap && n_live > 1;
    hipStream_t aux = nullptr;
    if (ov) {
        ZK_TRY(ensure_aux_stream());
        aux = cx.aux_stream;
        if (!cx.sort_ev[0]) for (int i = 0; i < 5; i++) ZK_HIP(hipEventCreateWithFlags(&cx.sort_ev[i], hipEventDisableTiming));
        ZK_HIP(hipEventRecord(cx.sort_ev[0], st));                   // the scalars are ready on the main stream at this point
        ZK_HIP(hipStreamWaitEvent(aux, cx.sort_ev[0], 0));
    }
    // r06: sort i and accumulation i are enqueued ALTERNATELY (sort 0, accumulation 0, sort 1, ...). Enqueueing every sort first left the main stream empty for
    // as long as the host needed to launch them (16 launches each: 0.35 ms between the end of sort 0 and the start of accumulation 0 in the kernel trace of a PLONK round).
    for (int i = 0; i < count; i++) {
        job[i] = MsmJob();
        if (ks[i] == 0) continue;
        ZK_TRY(msm_job_slot(i, job[i]));
        if (ov) {
            cx.stream = aux;
            int rc = msm_sort(d_scalars[i], ks[i], sb, pl[i], i, c, stride);
            if (!rc && hipEventRecord(cx.sort_ev[1 + i], aux) != hipSuccess) rc = fail(ZKMI_ERR_HIP, "hipEventRecord");
            cx.stream = st;
            ZK_TRY(rc);
            ZK_HIP(hipStreamWaitEvent(st, cx.sort_ev[1 + i], 0));
        } else ZK_TRY(msm_sort(d_scalars[i], ks[i], sb, pl[i], i, c, stride));
        ZK_TRY(msm_accumulate<F>(d_table, pl[i], 0, job[i]));
        jp[live++] = &job[i];
    }
    if (live) ZK_TRY(msm_reduce<F>(jp, live));
    ZK_HIP(hipEventRecord(cx.ev1, st));
    P.live = true; P.count = count; P.fw = FW;
    for (int i = 0; i < count; i++) P.ks[i] = ks[i];
    return ZKMI_OK;
}
template <class F> int msm_run_table_multi_collect(int count, uint8_t* out_jacs) {
    constexpr int FW = FieldWords<F>::value;
    Ctx& cx = ctx();
    MsmMultiPending& P = msm_multi_pending(cx.pipe);
    if (!P.live) return fail(ZKMI_ERR_INVALID, "msm_table_multi: nothing enqueued in this pipeline slot");
    if (P.fw != FW || P.count != count) { return fail(ZKMI_ERR_INVALID, "msm_table_multi: collect does not match what was enqueued (table or count)"); }
    P.live = false;
    ZK_HIP(hipStreamSynchronize(cx.stream));
    float ms = 0;
    if (hipEventElapsedTime(&ms, cx.ev0, cx.ev1) == hipSuccess) cx.last_ms = ms;
    for (int i = 0; i < P.count; i++) {
        if (P.ks[i] == 0) memset(out_jacs + (size_t)i * 12 * FW, 0, 12 * FW);
        else msm_fold<F>(P.job[i], out_jacs + (size_t)i * 12 * FW);
    }
    return ZKMI_OK;
}
template <class F> int msm_run_table_multi(const void* d_table, size_t stride, int c, const void* const* d_scalars, const size_t* ks, int count, size_t sb, uint8_t* out_jacs) {
    ZK_TRY(slot_idle_or_fail("msm_table_multi_dev"));                 // the one-call form abandons nothing: over an enqueued call it is refused like any other MSM
    int rc = msm_run_table_multi_enqueue<F>(d_table, stride, c, d_scalars, ks, count, sb);
    if (rc) { msm_multi_pending(ctx().pipe).live = false; return rc; }
    return msm_run_table_multi_collect<F>(count, out_jacs);
}

template <class F, class FrC> int gen_bases_run(const uint8_t* gen_affine_host, size_t n, uint64_t f, uint64_t g, void* d_out) {
    constexpr int FW = FieldWords<F>::value;
    Ctx& cx = ctx();
    uint32_t* d_gen;
    ZK_TRY(ws_get("gen.generator", 2 * FW * 4, (void**)&d_gen));
    ZK_HIP(hipMemcpyAsync(d_gen, gen_affine_host, 2 * FW * 4, hipMemcpyHostToDevice, cx.stream));
    hipLaunchKernelGGL((k_gen_geometric_bases<F, FrC>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, cx.stream, d_gen, (uint32_t)n, f, g, (uint32_t*)d_out);
    ZK_HIP(hipStreamSynchronize(cx.stream));
    ZK_HIP(hipGetLastError());
    return ZKMI_OK;
}

template <class F> int gen_scalar_bases_run(const uint8_t* gen_affine_host, const void* d_scalars, size_t n, void* d_out) {
    constexpr int FW = FieldWords<F>::value;
    Ctx& cx = ctx();
    uint32_t* d_gen;
    ZK_TRY(ws_get("gen.generator", 2 * FW * 4, (void**)&d_gen));
    ZK_HIP(hipMemcpyAsync(d_gen, gen_affine_host, 2 * FW * 4, hipMemcpyHostToDevice, cx.stream));
    hipLaunchKernelGGL((k_gen_scalar_bases<F>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, cx.stream, d_gen, (const uint32_t*)d_scalars, (uint32_t)n, (uint32_t*)d_out);
    ZK_HIP(hipStreamSynchronize(cx.stream));
    ZK_HIP(hipGetLastError());
    return ZKMI_OK;
}

}  // namespace zkmi
