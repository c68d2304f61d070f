// snarkjs_amd/csrc/aggregate_host.hpp — the kernels after the lane phase and the host side of the aggregated check (kzg_aggregate.cuh), shared by
// plonk_verify.hip and fflonk_verify.hip.
//
// One aggregated batch is: the protocol's lane kernel (one proof per lane; a block leaves ONE pair of partial sums, added up in LDS), then
// k_agg_reduce launches that each fold 64 pairs into one until a single pair is left (none up to 64 proofs, one up to 4 096, two up to 262 144),
// then k_agg_tail on one lane. Everything runs on the verifier's own stream, buffers and mutex (verify_host.hpp), under the same isolation
// rules as a per-proof batch; the partial sums live in two further buffers of the context, which only grow. No point arithmetic on the host:
// the host reads the codes and the tail's one-word verdict.
//
// KzgVerifyCtx is VerifyCtx (verify_host.hpp, unchanged) plus what an aggregated batch needs: two more events, the buffers of the partial sums and
// of the tail's report, and which kind of batch ran last. The Groth16 verifier uses it too, with kernels and records of its own
// (groth16_verify.hip, groth16_aggregate.cuh).
#pragma once
#include <string.h>
#include "verify_host.hpp"
#include "kzg_aggregate.cuh"

namespace zkmi {

struct AggSeed { uint64_t w[4]; };             // the 32 seed bytes as the sponge's first four lanes

template <class Entry> struct KzgVerifyCtx : VerifyCtx<Entry> {
    using Base = VerifyCtx<Entry>;
    hipEvent_t ev2 = nullptr, ev3 = nullptr;               // an aggregated batch: ev0 .. ev1 its lane phase, .. ev2 its reduction, .. ev3 its tail
    bool agg_last = false;                                 // the last timed batch was an aggregated one
    DevBuf agg_a, agg_b, agg_res;                          // partial sums (two levels of the tree), the tail's report

    int begin() {
        ZK_TRY(Base::begin());
        if (!ev2) {
            ZK_HIP(hipEventCreate(&ev2));
            ZK_HIP(hipEventCreate(&ev3));
        }
        return ZKMI_OK;
    }
    int release(uint64_t handle, const char* who) {
        ZK_TRY(begin());
        return Base::release(handle, who);
    }
    template <class Launch>
    int run_batch(const void* a, size_t a_bytes, const void* b, size_t b_bytes, void* host_out, size_t out_bytes, void* trace_out, size_t trace_bytes, bool time, Launch launch) {
        if (time) agg_last = false;
        return Base::run_batch(a, a_bytes, b, b_bytes, host_out, out_bytes, trace_out, trace_bytes, time, launch);
    }
    double last_ms() {
        if (!agg_last) return Base::last_ms();
        float ms = 0;
        if (!this->timed || hipEventElapsedTime(&ms, this->ev0, ev3) != hipSuccess) return -1.0;
        return ms;
    }
    // lane phase | reduction | tail of the last batch when it was an aggregated one
    int phase_ms(const char* who, double* out3) {
        if (!out3) return fail(ZKMI_ERR_INVALID, std::string(who) + ": null argument");
        hipEvent_t e[4] = {this->ev0, this->ev1, ev2, ev3};
        for (int i = 0; i < 3; i++) {
            float ms = 0;
            out3[i] = (this->timed && agg_last && hipEventElapsedTime(&ms, e[i], e[i + 1]) == hipSuccess) ? ms : -1.0;
        }
        return ZKMI_OK;
    }
};

// The lane phase, shared by the two protocols' lane kernels: one(i, pair) is the protocol's *_verify_one<C, true> on proof i. A lane that passes
// contributes r_i times its pair; lanes beyond n, and lanes whose input checks fail, the point at infinity. The block's pairs are added in sh
// (VERIFY_BLOCK entries of LDS) and leave as one.
template <class C, class One> __device__ __forceinline__ void agg_lane(AggPair<C>* sh, uint64_t n, const AggSeed& seed, int8_t* out, AggPair<C>* parts, One one) {
    const uint64_t i = (uint64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    AggPair<C> mine;
    pt_set_inf(mine.p);
    pt_set_inf(mine.q);
    if (i < n) {
        KzgPair<C> pr;
        const int code = one(i, &pr);
        if (code == AGG_ENTERED) {
            uint64_t lo, hi;
            agg_challenge(seed.w, i, lo, hi);
            mine.p = agg_scale<C>(pr.px, pr.py, pr.p_fin, lo, hi);
            mine.q = agg_scale<C>(pr.qx, pr.qy, pr.q_fin, lo, hi);
        }
        out[i] = (int8_t)code;
    }
    agg_block_sum<C, VERIFY_BLOCK>(sh, threadIdx.x, mine);
    if (threadIdx.x == 0) parts[blockIdx.x] = sh[0];
}

template <class C> __global__ void __launch_bounds__(VERIFY_BLOCK) k_agg_reduce(const AggPair<C>* in, uint64_t m, AggPair<C>* out) {
    __shared__ AggPair<C> sh[VERIFY_BLOCK];
    const uint64_t i = (uint64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    AggPair<C> mine;
    pt_set_inf(mine.p);
    pt_set_inf(mine.q);
    if (i < m) mine = in[i];
    agg_block_sum<C, VERIFY_BLOCK>(sh, threadIdx.x, mine);
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}

// x2_inf: the key's "X_2 is the point at infinity" word; x2_is_t0: X_2 is T0 (PLONK) or T1 (FFLONK)
template <class C> __global__ void __launch_bounds__(64) k_agg_tail(const AggPair<C>* S, const Line<C>* tab0, const Line<C>* tab1, const uint32_t* x2_inf, int x2_is_t0,
                                                                    const PairingConsts<C>* K, AggResult<C>* out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const bool x2_fin = *x2_inf == 0;
    agg_tail(*S, tab0, tab1, x2_is_t0 ? x2_fin : true, x2_is_t0 ? true : x2_fin, K, out);
}

// One aggregated batch of n > 0 proofs. lane(blocks, parts) launches the protocol's lane kernel on v.stream: it reads v.in_a / v.in_b, writes the
// n codes to v.out and one pair per block to parts. codes (n) and *ok are filled; sums (may be null) receives S_P | S_Q, 4 * C::N words.
template <class C, class Ctx, class Lane>
int run_aggregate(Ctx& v, const void* proofs, size_t a_bytes, const void* publics, size_t b_bytes, size_t n, int8_t* codes, int* ok, uint8_t* sums, const Line<C>* tab0,
                  const Line<C>* tab1, const uint32_t* x2_inf, int x2_is_t0, const PairingConsts<C>* K, Lane lane) {
    const unsigned blocks = verify_grid(n);
    ZK_TRY(grow(v.in_a, a_bytes));
    ZK_TRY(grow(v.in_b, b_bytes + 32));
    ZK_TRY(grow(v.out, n));
    ZK_TRY(grow(v.agg_a, (size_t)blocks * sizeof(AggPair<C>)));
    ZK_TRY(grow(v.agg_b, (size_t)verify_grid(blocks) * sizeof(AggPair<C>)));
    ZK_TRY(grow(v.agg_res, sizeof(AggResult<C>)));
    ZK_HIP(hipMemcpyAsync(v.in_a.p, proofs, a_bytes, hipMemcpyHostToDevice, v.stream));
    if (b_bytes) ZK_HIP(hipMemcpyAsync(v.in_b.p, publics, b_bytes, hipMemcpyHostToDevice, v.stream));
    ZK_HIP(hipEventRecord(v.ev0, v.stream));
    AggPair<C>* src = (AggPair<C>*)v.agg_a.p;
    AggPair<C>* dst = (AggPair<C>*)v.agg_b.p;
    lane(blocks, src);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipEventRecord(v.ev1, v.stream));
    for (unsigned m = blocks; m > 1;) {
        const unsigned g = verify_grid(m);
        hipLaunchKernelGGL(k_agg_reduce<C>, dim3(g), dim3(VERIFY_BLOCK), 0, v.stream, (const AggPair<C>*)src, (uint64_t)m, dst);
        ZK_HIP(hipGetLastError());
        AggPair<C>* t = src; src = dst; dst = t;
        m = g;
    }
    ZK_HIP(hipEventRecord(v.ev2, v.stream));
    hipLaunchKernelGGL(k_agg_tail<C>, dim3(1), dim3(64), 0, v.stream, (const AggPair<C>*)src, tab0, tab1, x2_inf, x2_is_t0, K, (AggResult<C>*)v.agg_res.p);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipEventRecord(v.ev3, v.stream));
    v.timed = true;
    v.agg_last = true;
    // res is on this frame: whatever the copies return, the stream is idle before the function is left
    AggResult<C> res;
    hipError_t copied = hipMemcpyAsync(codes, v.out.p, n, hipMemcpyDeviceToHost, v.stream);
    if (copied == hipSuccess) copied = hipMemcpyAsync(&res, v.agg_res.p, sizeof res, hipMemcpyDeviceToHost, v.stream);
    const hipError_t idle = hipStreamSynchronize(v.stream);
    ZK_HIP(copied);
    ZK_HIP(idle);
    bool all = res.pair_ok != 0;
    for (size_t i = 0; i < n; i++) all = all && codes[i] == AGG_ENTERED;
    *ok = all ? 1 : 0;
    if (sums) {
        memcpy(sums, res.sp, 8 * C::N);
        memcpy(sums + 8 * C::N, res.sq, 8 * C::N);
    }
    return ZKMI_OK;
}

}  // namespace zkmi
