// snarkjs_amd/csrc/ptau_challenge.hip — host driver + C-ABI of the challenge / response round trip of phase 1 (powersOfTau.challengeContribute / importResponse;
// ptau_challenge.cuh): the per-lane-scalar G2 multiplication, one section of a response from one upload of U-form points, and one section of an
// import from one upload of C-form points.
#include <string.h>
#include "ptau_challenge.cuh"
#include "host_field.hpp"
#include "msm_host.hpp"
#include "setup_common.hpp"
#include "zkmi_common.hpp"

namespace zkmi {

// csrc/ptau_contribute.hip: the slice of zkmi_diag_set_ptau_slice and the G1 kernel on prepared scalars
size_t ptau_slice_points();
int ptau_mul_each_g1(int curve, const void* d_in, const void* d_scalars, void* d_out, size_t n);

namespace {

struct Ones { uint32_t w[8]; };
__global__ void __launch_bounds__(256) k_ptauch_fill(uint32_t* __restrict__ dst, uint32_t n, const Ones one) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    reinterpret_cast<uint4*>(dst)[2 * (size_t)i] = make_uint4(one.w[0], one.w[1], one.w[2], one.w[3]);
    reinterpret_cast<uint4*>(dst)[2 * (size_t)i + 1] = make_uint4(one.w[4], one.w[5], one.w[6], one.w[7]);
}

host::HField<4> fr_of(int curve) { return curve == ZKMI_CURVE_BN128 ? host::HField<4>::from_cfg<Bn254Fr>() : host::HField<4>::from_cfg<Bls12381Fr>(); }

// C: the base field as the kernels see it; the 14-limb curve runs with CALLED products, as k_group_mul_each does and for its reason
template <class C> int mul_each_g2_run(const void* d_in, const void* d_scalars, void* d_out, size_t n) {
    Ctx& cx = ctx();
    constexpr int T = MulEachG2<C>::T;
    constexpr size_t lds = MulEachG2<C>::lds_bytes;
    ZK_TRY(lds_opt_in<k_group2_mul_each<C>>(lds));                  // dynamic LDS above the default limit
    uint32_t* work;
    ZK_TRY(ws_get("ptauch.work", n * 8 * C::N * 4, (void**)&work));
    ZK_HIP(hipEventRecord(cx.ev0, cx.stream));
    hipLaunchKernelGGL((k_group2_mul_each<C>), dim3((unsigned)((n + T - 1) / T)), dim3(T), lds, cx.stream, (const uint32_t*)d_in, (const uint32_t*)d_scalars, work, (uint32_t)n);
    const size_t groups = (n + SCALE_INV - 1) / SCALE_INV;
    hipLaunchKernelGGL((k_group2_scale_affine<C>), dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, cx.stream, work, (uint32_t*)d_out, (uint32_t)n);
    ZK_HIP(hipEventRecord(cx.ev1, cx.stream));
    ZK_HIP(hipGetLastError());
    return ZKMI_OK;
}
int mul_each_g2_dispatch(int curve, const void* d_in, const void* d_scalars, void* d_out, size_t n) {
    return curve == ZKMI_CURVE_BN128 ? mul_each_g2_run<Bn254Fq>(d_in, d_scalars, d_out, n) : mul_each_g2_run<Compact<Bls12381Fq>>(d_in, d_scalars, d_out, n);
}

// points [0, n) of a section that starts at scalar `first`, as contribute_g1 of ptau_contribute.hip cuts and prepares them: slices of at most
// ptau_slice_points() points, the scalars of a slice made on the device from a buffer of ones (first_s * inc^i by the Fr batchApplyKey kernel, then out of
// Montgomery form), first_s = first * inc^(slice start) from the host; the slice goes to the kernel of its group
int mul_each_sliced(int curve, int group, const uint8_t* d_in, uint8_t* d_out, size_t n, const uint8_t* first, const uint8_t* inc) {
    Ctx& cx = ctx();
    const host::HField<4> Fr = fr_of(curve);
    const size_t limit = ptau_slice_points();
    const size_t sG = (size_t)2 * group * n8q_of(curve), slice = limit < n ? limit : n;
    uint32_t *d_ones, *d_scal;
    ZK_TRY(ws_get("ptauch.ones", slice * 32, (void**)&d_ones));
    ZK_TRY(ws_get("ptauch.scalars", slice * 32, (void**)&d_scal));
    Ones one;
    const host::HFp<4> o = Fr.One();
    memcpy(one.w, o.v, 32);
    hipLaunchKernelGGL(k_ptauch_fill, dim3((unsigned)((slice + 255) / 256)), dim3(256), 0, cx.stream, d_ones, (uint32_t)slice, one);
    ZK_HIP(hipGetLastError());
    host::HFp<4> f, step;
    memcpy(f.v, first, 32);
    memcpy(step.v, inc, 32);
    const host::HFp<4> jump = Fr.pow_u64(step, (uint64_t)slice);
    for (size_t at = 0; at < n; at += slice) {
        const size_t m = n - at < slice ? n - at : slice;
        ZK_TRY(apply_key_dev_dispatch(curve, d_ones, d_scal, m, (const uint8_t*)f.v, inc));
        ZK_TRY(fr_batch_dev_dispatch(curve, ZKMI_BATCH_FROM_MONTGOMERY, d_scal, d_scal, m));
        if (group == 1) ZK_TRY(ptau_mul_each_g1(curve, d_in + at * sG, d_scal, d_out + at * sG, m));
        else ZK_TRY(mul_each_g2_dispatch(curve, d_in + at * sG, d_scal, d_out + at * sG, m));
        f = Fr.mul(f, jump);
    }
    return ZKMI_OK;
}

int pages_check(const char* who, const char* what, uint8_t* const* ptr, const size_t* len, int n_pages, size_t bytes) {
    if (!ptr || !len || n_pages < 0) return fail(ZKMI_ERR_INVALID, std::string(who) + ": null argument");
    size_t cap = 0;
    for (int i = 0; i < n_pages; i++) {
        if (len[i] && !ptr[i]) return fail(ZKMI_ERR_INVALID, std::string(who) + ": null argument");
        cap += len[i];
    }
    if (cap != bytes) return fail(ZKMI_ERR_INVALID, std::string(who) + ": the " + what + " pages do not hold n points");
    return ZKMI_OK;
}

}  // namespace
}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zkmi_diag_group2_mul_each_dev(int curve, const void* d_points, const void* d_scalars_normal, void* d_out, size_t n) {
    ZK_TRY(require_ctx());
    if (curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) return fail(ZKMI_ERR_INVALID, "group mul each: unknown curve or group");
    if (pipeline_busy()) return fail(ZKMI_ERR_INVALID, "group mul each: a pipeline slot holds work in flight (collect it first)");
    if (!n) return ZKMI_OK;
    if (!d_points || !d_scalars_normal || !d_out) return fail(ZKMI_ERR_INVALID, "group mul each: null buffer");
    if (n >= (1ull << 31)) return fail(ZKMI_ERR_UNSUPPORTED, "group mul each: at most 2^31 - 1 points");
    return mul_each_g2_dispatch(curve, d_points, d_scalars_normal, d_out, n);
}

int zkmi_ptau_challenge_section(int curve, int group, zkmi_pages in_u, size_t n, const uint8_t* first, const uint8_t* inc, uint8_t* const* out_ptr, const size_t* out_len,
                                int n_out_pages, int form) {
    static const char* const who = "ptau_challenge_section";
    ZK_TRY(require_ctx());
    if ((curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) || (group != 1 && group != 2) || (form != 0 && form != 1))
        return fail(ZKMI_ERR_INVALID, "ptau_challenge_section: unknown curve, group or form");
    if (!first || !inc) return fail(ZKMI_ERR_INVALID, "ptau_challenge_section: null argument");
    if (pipeline_busy()) return fail(ZKMI_ERR_INVALID, "ptau_challenge_section: a pipeline slot holds work in flight (collect it first)");
    if (!n) return ZKMI_OK;
    if (n >= (1ull << 31)) return fail(ZKMI_ERR_UNSUPPORTED, "ptau_challenge_section: at most 2^31 - 1 points");
    const size_t sG = (size_t)2 * group * n8q_of(curve), bytes = n * sG, out_bytes = form == 0 ? bytes / 2 : bytes;
    if (!in_u.ptr || !in_u.len) return fail(ZKMI_ERR_INVALID, "ptau_challenge_section: null argument");
    if (pages_bytes(in_u) != bytes) return fail(ZKMI_ERR_INVALID, "ptau_challenge_section: the input pages do not hold n points");
    ZK_TRY(pages_check(who, "output", out_ptr, out_len, n_out_pages, out_bytes));
    DevMem dm(who);
    uint8_t *d_in, *d_lem;
    ZK_TRY(dm.get(bytes, (void**)&d_in));
    ZK_TRY(dm.get(bytes, (void**)&d_lem));
    ZK_TRY(upload_pages(in_u, bytes, d_in));
    ZK_TRY(zkmi_group_convert_dev(curve, group, ZKMI_CONV_U_TO_LEM, d_in, d_lem, n));
    ZK_TRY(mul_each_sliced(curve, group, d_lem, d_in, n, first, inc));                  // the upload's buffer takes the products: source and destination distinct
    ZK_TRY(zkmi_group_convert_dev(curve, group, form == 0 ? ZKMI_CONV_LEM_TO_C : ZKMI_CONV_LEM_TO_U, d_in, d_lem, n));
    return download_pages(d_lem, out_bytes, out_ptr, out_len, n_out_pages);
}

int zkmi_ptau_import_section(int curve, int group, zkmi_pages in_c, size_t n, uint8_t* const* lem_ptr, const size_t* lem_len, int n_lem_pages, uint8_t* const* u_ptr,
                             const size_t* u_len, int n_u_pages) {
    static const char* const who = "ptau_import_section";
    ZK_TRY(require_ctx());
    if ((curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) || (group != 1 && group != 2)) return fail(ZKMI_ERR_INVALID, "ptau_import_section: unknown curve or group");
    if (pipeline_busy()) return fail(ZKMI_ERR_INVALID, "ptau_import_section: a pipeline slot holds work in flight (collect it first)");
    if (!n) return ZKMI_OK;
    if (n >= (1ull << 31)) return fail(ZKMI_ERR_UNSUPPORTED, "ptau_import_section: at most 2^31 - 1 points");
    const size_t sG = (size_t)2 * group * n8q_of(curve), bytes = n * sG;
    if (!in_c.ptr || !in_c.len) return fail(ZKMI_ERR_INVALID, "ptau_import_section: null argument");
    if (pages_bytes(in_c) != bytes / 2) return fail(ZKMI_ERR_INVALID, "ptau_import_section: the input pages do not hold n points");
    ZK_TRY(pages_check(who, "LEM output", lem_ptr, lem_len, n_lem_pages, bytes));
    ZK_TRY(pages_check(who, "U output", u_ptr, u_len, n_u_pages, bytes));
    DevMem dm(who);
    uint8_t *d_in, *d_lem;
    ZK_TRY(dm.get(bytes, (void**)&d_in));                                               // the C form first, the U form afterwards
    ZK_TRY(dm.get(bytes, (void**)&d_lem));
    ZK_TRY(upload_pages(in_c, bytes / 2, d_in));
    ZK_TRY(zkmi_group_convert_dev(curve, group, ZKMI_CONV_C_TO_LEM, d_in, d_lem, n));   // ZKMI_ERR_INVALID when some x has no point on the curve
    ZK_TRY(download_pages(d_lem, bytes, lem_ptr, lem_len, n_lem_pages));
    ZK_TRY(zkmi_group_convert_dev(curve, group, ZKMI_CONV_LEM_TO_U, d_lem, d_in, n));
    return download_pages(d_in, bytes, u_ptr, u_len, n_u_pages);
}

}  // extern "C"
