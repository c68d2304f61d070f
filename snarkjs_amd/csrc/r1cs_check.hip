// snarkjs_amd/csrc/r1cs_check.hip — snarkjs.wtns.check (reference src/wtns_check.js: one JavaScript loop over the constraints) on the device.
//
//   zkmi_r1cs_load       r1cs section 2 -> the resident sliced layout of its 3 * nConstraints linear combinations (r1cs_check.cuh, abc_layout.cuh): a host pass
//                        over the term counts alone (r1cs_host.hpp), one upload of the raw section and the prefix array, everything else on the device
//   zkmi_r1cs_check(_dev) a batch of witnesses against it: reduce the witness values, walk the layout (grid y = witness), fold the cut rows in the same
//                        launch, A B == C per (witness, constraint), first failing constraint per witness
// Both run on the active pipeline slot's stream and compute no MSM: they are not refused while a slot holds work in flight. The work memory belongs to the
// key and every check ends with a synchronisation of the stream it ran on, so one key serves one check at a time, as the library serves one caller.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <memory>
#include "r1cs_check.cuh"
#include "r1cs_host.hpp"
#include "zkmi_common.hpp"

namespace zkmi {

namespace {

constexpr uint64_t R1CS_BUDGET_DEFAULT = 4ull << 30;     // work memory of one pass over a batch
constexpr uint32_t R1CS_GRID_Y = 65535;
uint64_t g_budget = R1CS_BUDGET_DEFAULT;

struct Tmp {                                              // device memory of one load: freed on every return path
    void* p = nullptr;
    ~Tmp() { if (p) (void)hipFree(p); }
};

struct R1csKey {
    int curve = 0;
    uint32_t n_constraints = 0, n_vars = 0, n_terms = 0;
    uint64_t used = 0;                                    // bytes of section 2 the constraints take
    uint32_t *s_len = nullptr, *s_out = nullptr, *slice_off = nullptr, *sell_sig = nullptr, *sell_val = nullptr, *long_rows = nullptr, *part_row = nullptr;
    uint32_t n_seg = 0, n_long = 0, n_part = 0;
    // work memory of a pass over `cap` witnesses: witnesses as given (host entry), reduced, evaluations, partial sums, tickets, verdicts
    uint32_t cap = 0;
    uint32_t *w_in = nullptr, *w_red = nullptr, *ev = nullptr, *part = nullptr, *cnt = nullptr, *bad = nullptr;
    uint64_t per_witness() const { return 32ull * n_vars + 96ull * n_constraints + 32ull * n_part + 4ull * n_long + 4; }
    void free_work() {
        for (uint32_t** p : {&w_in, &w_red, &ev, &part, &cnt, &bad}) if (*p) { (void)hipFree(*p); *p = nullptr; }
        cap = 0;
    }
    ~R1csKey() {
        free_work();
        for (uint32_t** p : {&s_len, &s_out, &slice_off, &sell_sig, &sell_val, &long_rows, &part_row}) if (*p) (void)hipFree(*p);
    }
    R1csKey() = default;
    R1csKey(const R1csKey&) = delete;
    R1csKey& operator=(const R1csKey&) = delete;
};
std::map<uint64_t, std::unique_ptr<R1csKey>> g_keys;

// the layout of abc_layout.cuh over rows = 3 * constraint + matrix, as g16_build_sell (groth16.hip) builds it over section 4, then the terms
template <class C> int build_layout(R1csKey& K, const zkmi_pages& constraints, const std::vector<uint32_t>& lc_first, hipStream_t st) {
    const size_t rows = 3 * (size_t)K.n_constraints;
    const uint32_t n_terms = K.n_terms;
    Tmp raw_t, first_t, cnt_t, nseg_t, npart_t, segb_t, partb_t, seglen_t, segout_t, counts_t, offs_t, pos_t, slw_t, misc_t, mark_t;
    ZK_HIP(hipMalloc(&raw_t.p, (size_t)K.used + 16));
    ZK_TRY(upload_pages(constraints, (size_t)K.used, raw_t.p));
    ZK_HIP(hipMalloc(&first_t.p, (rows + 1) * 4 + 16));
    ZK_HIP(hipMemcpyAsync(first_t.p, lc_first.data(), (rows + 1) * 4, hipMemcpyHostToDevice, st));
    const uint32_t *raw = (const uint32_t*)raw_t.p, *d_first = (const uint32_t*)first_t.p;
    for (Tmp* t : {&cnt_t, &nseg_t, &npart_t, &segb_t, &partb_t, &mark_t}) ZK_HIP(hipMalloc(&t->p, rows * 4 + 16));
    ZK_HIP(hipMalloc(&misc_t.p, 64));                                   // [0] flags of the fill, [1] cut rows, [2] adjacent pairs out of order
    uint32_t *row_cnt = (uint32_t*)cnt_t.p, *nseg = (uint32_t*)nseg_t.p, *npart = (uint32_t*)npart_t.p, *seg_base = (uint32_t*)segb_t.p, *part_base = (uint32_t*)partb_t.p,
             *marked = (uint32_t*)mark_t.p, *misc = (uint32_t*)misc_t.p;
    ZK_HIP(hipMemsetAsync(misc, 0, 64, st)); ZK_HIP(hipMemsetAsync(marked, 0, rows * 4, st));
    const unsigned tblocks = (unsigned)(((uint64_t)n_terms + 255) / 256), rblocks = (unsigned)((rows + 255) / 256);
    hipLaunchKernelGGL(k_r1cs_row_cnt, dim3(rblocks), dim3(256), 0, st, d_first, (uint32_t)rows, row_cnt);
    hipLaunchKernelGGL(k_abc_row_segs, dim3(rblocks), dim3(256), 0, st, row_cnt, (uint32_t)rows, nseg, npart);
    hipLaunchKernelGGL(k_scan_u32, dim3(1), dim3(1024), 0, st, nseg, seg_base, (uint32_t)rows);
    hipLaunchKernelGGL(k_scan_u32, dim3(1), dim3(1024), 0, st, npart, part_base, (uint32_t)rows);
    uint32_t tail[4] = {0, 0, 0, 0};                                    // last seg_base, last nseg, last part_base, last npart
    ZK_HIP(hipMemcpyAsync(&tail[0], seg_base + rows - 1, 4, hipMemcpyDeviceToHost, st)); ZK_HIP(hipMemcpyAsync(&tail[1], nseg + rows - 1, 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(&tail[2], part_base + rows - 1, 4, hipMemcpyDeviceToHost, st)); ZK_HIP(hipMemcpyAsync(&tail[3], npart + rows - 1, 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    const size_t n_seg = (size_t)tail[0] + tail[1], n_part = (size_t)tail[2] + tail[3];
    if (n_seg >= 0x7fffffffu || n_part >= 0x7fffffffu) return fail(ZKMI_ERR_UNSUPPORTED, "r1cs_load: constraint section too large for the 31-bit segment indices");
    K.n_seg = (uint32_t)n_seg; K.n_part = (uint32_t)n_part;
    const uint32_t n_waves = (uint32_t)((n_seg + 63) / 64);             // = slices
    ZK_HIP(hipMalloc(&seglen_t.p, n_seg * 4 + 16)); ZK_HIP(hipMalloc(&segout_t.p, n_seg * 4 + 16)); ZK_HIP(hipMalloc(&pos_t.p, n_seg * 4 + 16));
    const size_t n_counts = (size_t)(ABC_SEG + 1) * n_waves;
    if (n_counts >= 0xffffffffu) return fail(ZKMI_ERR_UNSUPPORTED, "r1cs_load: constraint section too large for the segment sort");
    ZK_HIP(hipMalloc(&counts_t.p, n_counts * 4 + 16)); ZK_HIP(hipMalloc(&offs_t.p, n_counts * 4 + 16)); ZK_HIP(hipMalloc(&slw_t.p, (size_t)n_waves * 4 + 16));
    ZK_HIP(hipMalloc((void**)&K.long_rows, (size_t)(n_terms / (ABC_SEG + 1) + 1) * 12));
    ZK_HIP(hipMalloc((void**)&K.part_row, std::max<size_t>(n_part, 1) * 4));
    ZK_TRY(dev_alloc_big((void**)&K.s_len, n_seg * 4 + 16)); ZK_TRY(dev_alloc_big((void**)&K.s_out, n_seg * 4 + 16));
    ZK_HIP(hipMalloc((void**)&K.slice_off, (size_t)n_waves * 4 + 16));
    uint32_t *seg_len = (uint32_t*)seglen_t.p, *seg_out = (uint32_t*)segout_t.p, *pos_of_seg = (uint32_t*)pos_t.p, *counts = (uint32_t*)counts_t.p, *offs = (uint32_t*)offs_t.p,
             *slice_w = (uint32_t*)slw_t.p;
    hipLaunchKernelGGL(k_abc_seg_fill, dim3(rblocks), dim3(256), 0, st, row_cnt, seg_base, part_base, (uint32_t)rows, seg_len, seg_out, K.long_rows, misc + 1);
    ZK_HIP(hipMemsetAsync(counts, 0, n_counts * 4, st));
    hipLaunchKernelGGL(k_abc_wave_hist, dim3(n_waves), dim3(64), 0, st, seg_len, (uint32_t)n_seg, n_waves, counts);
    hipLaunchKernelGGL(k_scan_u32, dim3(1), dim3(1024), 0, st, counts, offs, (uint32_t)n_counts);
    hipLaunchKernelGGL(k_abc_wave_rank, dim3(n_waves), dim3(64), 0, st, seg_len, seg_out, (uint32_t)n_seg, n_waves, offs, K.s_len, K.s_out, pos_of_seg);
    hipLaunchKernelGGL(k_abc_slice_w, dim3((n_waves + 255) / 256), dim3(256), 0, st, K.s_len, n_waves, slice_w);
    hipLaunchKernelGGL(k_scan_u32, dim3(1), dim3(1024), 0, st, slice_w, K.slice_off, n_waves);
    if (n_terms) hipLaunchKernelGGL(k_r1cs_dup_mark, dim3(tblocks), dim3(256), 0, st, raw, d_first, (uint32_t)rows, n_terms, marked, misc + 2);
    uint32_t t2[4] = {0, 0, 0, 0};                                      // cut rows, last slice_off, last slice_w, adjacent pairs out of order
    ZK_HIP(hipMemcpyAsync(&t2[0], misc + 1, 4, hipMemcpyDeviceToHost, st)); ZK_HIP(hipMemcpyAsync(&t2[3], misc + 2, 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(&t2[1], K.slice_off + n_waves - 1, 4, hipMemcpyDeviceToHost, st)); ZK_HIP(hipMemcpyAsync(&t2[2], slice_w + n_waves - 1, 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    K.n_long = t2[0];
    const size_t sell_terms = ((size_t)t2[1] + t2[2]) * 64;
    ZK_TRY(dev_alloc_big((void**)&K.sell_sig, std::max<size_t>(sell_terms, 1) * 4)); ZK_TRY(dev_alloc_big((void**)&K.sell_val, std::max<size_t>(sell_terms, 1) * 32));
    if (K.n_long) hipLaunchKernelGGL(k_r1cs_part_row, dim3((K.n_long + 255) / 256), dim3(256), 0, st, K.long_rows, K.n_long, K.part_row);
    if (n_terms) hipLaunchKernelGGL((k_r1cs_fill<C>), dim3(tblocks), dim3(256), 0, st, raw, d_first, (uint32_t)rows, n_terms, K.n_vars, seg_base, pos_of_seg, K.slice_off, K.sell_sig,
                                    K.sell_val, misc);
    if (n_terms && t2[3]) hipLaunchKernelGGL(k_r1cs_dup_fix, dim3(tblocks), dim3(256), 0, st, raw, d_first, (uint32_t)rows, n_terms, marked, seg_base, pos_of_seg, K.slice_off, K.sell_val);
    uint32_t flags = 0;
    ZK_HIP(hipMemcpyAsync(&flags, misc, 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    if (flags & R1CS_FLAG_SIGNAL) return fail(ZKMI_ERR_INVALID, "r1cs_load: a constraint names a signal beyond nVars");
    return ZKMI_OK;
}

int ensure_work(R1csKey& K, uint32_t cap, bool host_in) {
    if (K.cap < cap) {
        K.free_work();
        ZK_TRY(dev_alloc_big((void**)&K.w_red, std::max<size_t>((size_t)cap * K.n_vars, 1) * 32));
        ZK_TRY(dev_alloc_big((void**)&K.ev, std::max<size_t>((size_t)cap * K.n_constraints * 3, 1) * 32));
        ZK_TRY(dev_alloc_big((void**)&K.part, std::max<size_t>((size_t)cap * K.n_part, 1) * 32));
        ZK_HIP(hipMalloc((void**)&K.cnt, std::max<size_t>((size_t)cap * K.n_long, 1) * 4));
        ZK_HIP(hipMalloc((void**)&K.bad, (size_t)cap * 4));
        K.cap = cap;
    }
    if (host_in && !K.w_in) ZK_TRY(dev_alloc_big((void**)&K.w_in, std::max<size_t>((size_t)K.cap * K.n_vars, 1) * 32));
    return ZKMI_OK;
}

// one pass: kb witnesses in device memory -> first_bad[0 .. kb) on the host
template <class C> int check_pass(R1csKey& K, const uint32_t* d_w, uint32_t kb, uint32_t* first_bad, hipStream_t st) {
    const size_t count = (size_t)kb * K.n_vars;
    ZK_HIP(hipMemsetAsync(K.bad, 0xff, (size_t)kb * 4, st));
    if (K.n_constraints) {
        if (count) hipLaunchKernelGGL((k_r1cs_reduce_w<C>), dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, d_w, K.w_red, count);
        if (K.n_long) ZK_HIP(hipMemsetAsync(K.cnt, 0, (size_t)kb * K.n_long * 4, st));
        hipLaunchKernelGGL((k_r1cs_sell<C>), dim3((K.n_seg + 255) / 256, kb), dim3(256), 0, st, K.s_len, K.s_out, K.slice_off, K.n_seg, K.sell_sig, K.sell_val, K.w_red, K.n_vars, K.ev,
                           3 * K.n_constraints, K.part, K.n_part, K.long_rows, K.n_long, K.part_row, K.cnt);
        hipLaunchKernelGGL((k_r1cs_verdict<C>), dim3((K.n_constraints + 255) / 256, kb), dim3(256), 0, st, K.ev, K.n_constraints, K.bad);
    }
    ZK_HIP(hipMemcpyAsync(first_bad, K.bad, (size_t)kb * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    return ZKMI_OK;
}

int check_run(uint64_t key, const void* witnesses, size_t witness_len, uint32_t n_witnesses, uint32_t* first_bad, bool host_in, const char* who) {
    ZK_TRY(require_ctx());
    if (key == 0) return fail(ZKMI_ERR_INVALID, std::string(who) + ": cache key 0 names no resident r1cs");
    auto it = g_keys.find(key);
    if (it == g_keys.end()) return fail(ZKMI_ERR_INVALID, std::string(who) + ": no r1cs is resident under this key (zkmi_r1cs_load)");
    R1csKey& K = *it->second;
    if (n_witnesses == 0) return witness_len == 0 ? ZKMI_OK : fail(ZKMI_ERR_INVALID, std::string(who) + ": witness_len is not n_witnesses x nVars x 32");
    if (!witnesses || !first_bad) return fail(ZKMI_ERR_INVALID, std::string(who) + ": null pointer");
    if ((uint64_t)witness_len != 32ull * K.n_vars * n_witnesses) return fail(ZKMI_ERR_INVALID, std::string(who) + ": witness_len is not n_witnesses x nVars x 32");
    hipStream_t st = ctx().stream;
    const uint32_t cut = r1cs_batch_cut(K.per_witness(), n_witnesses, g_budget, R1CS_GRID_Y);
    ZK_TRY(ensure_work(K, cut, host_in));
    const size_t one = (size_t)K.n_vars * 32;
    for (uint32_t k0 = 0; k0 < n_witnesses; k0 += cut) {
        const uint32_t kb = std::min(cut, n_witnesses - k0);
        const uint8_t* src = (const uint8_t*)witnesses + (size_t)k0 * one;
        if (host_in) ZK_HIP(hipMemcpyAsync(K.w_in, src, (size_t)kb * one, hipMemcpyHostToDevice, st));
        const uint32_t* d_w = host_in ? K.w_in : (const uint32_t*)src;
        ZK_TRY(K.curve == ZKMI_CURVE_BN128 ? check_pass<Bn254Fr>(K, d_w, kb, first_bad + k0, st) : check_pass<Bls12381Fr>(K, d_w, kb, first_bad + k0, st));
    }
    return ZKMI_OK;
}

}  // namespace

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zkmi_r1cs_load(int curve, zkmi_pages constraints, uint32_t n_constraints, uint32_t n_vars, uint64_t cache_key) {
    ZK_TRY(require_ctx());
    if (curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) return fail(ZKMI_ERR_INVALID, "r1cs_load: unknown curve");
    if (cache_key == 0) return fail(ZKMI_ERR_INVALID, "r1cs_load: cache key 0 names no resident r1cs");
    if (constraints.n_pages < 0 || (constraints.n_pages > 0 && (!constraints.ptr || !constraints.len))) return fail(ZKMI_ERR_INVALID, "r1cs_load: null pointer");
    for (int i = 0; i < constraints.n_pages; i++) if (constraints.len[i] && !constraints.ptr[i]) return fail(ZKMI_ERR_INVALID, "r1cs_load: null pointer");
    if (3ull * n_constraints >= (1ull << 31)) return fail(ZKMI_ERR_UNSUPPORTED, "r1cs_load: 3 x nConstraints does not fit 31 bits");
    std::vector<uint32_t> lc_first;
    uint64_t used = 0;
    const int rc = r1cs_lc_offsets(constraints, n_constraints, lc_first, &used);
    if (rc == R1CS_OFFSETS_SHORT) return fail(ZKMI_ERR_INVALID, "r1cs_load: the r1cs constraint section ends inside a constraint");
    if (rc == R1CS_OFFSETS_TOO_MANY) return fail(ZKMI_ERR_UNSUPPORTED, "r1cs_load: 2^32 terms or more");
    auto it = g_keys.find(cache_key);
    if (it != g_keys.end()) {
        const R1csKey& R = *it->second;
        if (R.curve == curve && R.n_constraints == n_constraints && R.n_vars == n_vars && R.used == used && R.n_terms == lc_first.back()) return ZKMI_OK;
        return fail(ZKMI_ERR_INVALID, "r1cs_load: another r1cs is resident under this key (zkmi_r1cs_release it first)");
    }
    auto K = std::make_unique<R1csKey>();
    K->curve = curve; K->n_constraints = n_constraints; K->n_vars = n_vars; K->used = used; K->n_terms = lc_first.back();
    if (n_constraints) ZK_TRY(curve == ZKMI_CURVE_BN128 ? build_layout<Bn254Fr>(*K, constraints, lc_first, ctx().stream) : build_layout<Bls12381Fr>(*K, constraints, lc_first, ctx().stream));
    g_keys[cache_key] = std::move(K);
    return ZKMI_OK;
}

int zkmi_r1cs_check(uint64_t cache_key, const uint8_t* witnesses, size_t witness_len, uint32_t n_witnesses, uint32_t* first_bad) {
    return check_run(cache_key, witnesses, witness_len, n_witnesses, first_bad, true, "r1cs_check");
}

int zkmi_r1cs_check_dev(uint64_t cache_key, const void* d_witnesses, size_t witness_len, uint32_t n_witnesses, uint32_t* first_bad) {
    return check_run(cache_key, d_witnesses, witness_len, n_witnesses, first_bad, false, "r1cs_check_dev");
}

int zkmi_r1cs_release(uint64_t cache_key) {
    auto it = g_keys.find(cache_key);
    if (it == g_keys.end()) return ZKMI_OK;
    if (ctx().ready) (void)hipStreamSynchronize(ctx().stream);
    g_keys.erase(it);
    return ZKMI_OK;
}

int zkmi_diag_set_r1cs_budget(size_t bytes) {
    g_budget = bytes ? (uint64_t)bytes : R1CS_BUDGET_DEFAULT;
    return ZKMI_OK;
}

}  // extern "C"
