// snarkjs_amd/csrc/ptau_contribute.hip — host driver + C-ABI of a phase-1 contribution (powersOfTau.contribute / beacon; ptau_contribute.cuh):
// the per-lane-scalar G1 multiplication, one section of a contribution from one upload, and the hasher state a contribution keeps (misc.toPartialHash).
#include <string.h>
#include "ptau_contribute.cuh"
#include "host_field.hpp"
#include "ptau_host.hpp"
#include "setup_common.hpp"
#include "zkmi_common.hpp"

namespace zkmi {
namespace {

constexpr size_t PTAU_SLICE_DEFAULT = (size_t)1 << 20;       // points per slice: bounds the XYZZ work array at 128 B x 2^20 (BN254)
size_t g_ptau_slice = PTAU_SLICE_DEFAULT;

struct Ones { uint32_t w[8]; };
__global__ void __launch_bounds__(256) k_ptauc_fill(uint32_t* __restrict__ dst, uint32_t n, const Ones one) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    reinterpret_cast<uint4*>(dst)[2 * (size_t)i] = make_uint4(one.w[0], one.w[1], one.w[2], one.w[3]);
    reinterpret_cast<uint4*>(dst)[2 * (size_t)i + 1] = make_uint4(one.w[4], one.w[5], one.w[6], one.w[7]);
}

host::HField<4> fr_of(int curve) { return curve == ZKMI_CURVE_BN128 ? host::HField<4>::from_cfg<Bn254Fr>() : host::HField<4>::from_cfg<Bls12381Fr>(); }

// C: the base field as the kernels see it; the 14-limb curve runs with CALLED products, as in group_scale.hip and for its reason: the loop must fit the
// instruction cache
template <class C> int mul_each_run(const void* d_in, const void* d_scalars, void* d_out, size_t n) {
    Ctx& cx = ctx();
    uint32_t* work;
    ZK_TRY(ws_get("ptauc.work", n * 4 * C::N * 4, (void**)&work));
    ZK_HIP(hipEventRecord(cx.ev0, cx.stream));
    hipLaunchKernelGGL((k_group_mul_each<C>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, cx.stream, (const uint32_t*)d_in, (const uint32_t*)d_scalars, work, (uint32_t)n);
    const size_t groups = (n + SCALE_INV - 1) / SCALE_INV;
    hipLaunchKernelGGL((k_group_scale_affine<C>), dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, cx.stream, work, (uint32_t*)d_out, (uint32_t)n);
    ZK_HIP(hipEventRecord(cx.ev1, cx.stream));
    ZK_HIP(hipGetLastError());
    return ZKMI_OK;
}
int mul_each_dispatch(int curve, const void* d_in, const void* d_scalars, void* d_out, size_t n) {
    return curve == ZKMI_CURVE_BN128 ? mul_each_run<Bn254Fq>(d_in, d_scalars, d_out, n) : mul_each_run<Compact<Bls12381Fq>>(d_in, d_scalars, d_out, n);
}

// G1 points [0, n) of a section that starts at scalar `first`: slices of at most g_ptau_slice points, the scalars of a slice made on the device from a
// buffer of ones (first_s * inc^i by the Fr batchApplyKey kernel, then out of Montgomery form), first_s = first * inc^(slice start) from the host
int contribute_g1(int curve, const uint8_t* d_in, uint8_t* d_out, size_t n, const uint8_t* first, const uint8_t* inc) {
    Ctx& cx = ctx();
    const host::HField<4> Fr = fr_of(curve);
    const size_t sG = (size_t)2 * n8q_of(curve), slice = g_ptau_slice < n ? g_ptau_slice : n;
    uint32_t *d_ones, *d_scal;
    ZK_TRY(ws_get("ptauc.ones", slice * 32, (void**)&d_ones));
    ZK_TRY(ws_get("ptauc.scalars", slice * 32, (void**)&d_scal));
    Ones one;
    const host::HFp<4> o = Fr.One();
    memcpy(one.w, o.v, 32);
    hipLaunchKernelGGL(k_ptauc_fill, dim3((unsigned)((slice + 255) / 256)), dim3(256), 0, cx.stream, d_ones, (uint32_t)slice, one);
    ZK_HIP(hipGetLastError());
    host::HFp<4> f, step;
    memcpy(f.v, first, 32);
    memcpy(step.v, inc, 32);
    const host::HFp<4> jump = Fr.pow_u64(step, (uint64_t)slice);
    for (size_t at = 0; at < n; at += slice) {
        const size_t m = n - at < slice ? n - at : slice;
        ZK_TRY(apply_key_dev_dispatch(curve, d_ones, d_scal, m, (const uint8_t*)f.v, inc));
        ZK_TRY(fr_batch_dev_dispatch(curve, ZKMI_BATCH_FROM_MONTGOMERY, d_scal, d_scal, m));
        ZK_TRY(mul_each_dispatch(curve, d_in + at * sG, d_scal, d_out + at * sG, m));
        f = Fr.mul(f, jump);
    }
    return ZKMI_OK;
}

int pages_check(const char* what, uint8_t* const* ptr, const size_t* len, int n_pages, size_t bytes) {
    if (!ptr || !len || n_pages < 0) return fail(ZKMI_ERR_INVALID, "ptau_contribute_section: null argument");
    size_t cap = 0;
    for (int i = 0; i < n_pages; i++) {
        if (len[i] && !ptr[i]) return fail(ZKMI_ERR_INVALID, "ptau_contribute_section: null argument");
        cap += len[i];
    }
    if (cap != bytes) return fail(ZKMI_ERR_INVALID, std::string("ptau_contribute_section: the ") + what + " pages do not hold n points");
    return ZKMI_OK;
}

}  // namespace

// for csrc/ptau_challenge.hip, whose section call cuts and runs its G1 slices as contribute_g1 does: the slice in force and the kernel on prepared scalars
size_t ptau_slice_points() { return g_ptau_slice; }
int ptau_mul_each_g1(int curve, const void* d_in, const void* d_scalars, void* d_out, size_t n) { return mul_each_dispatch(curve, d_in, d_scalars, d_out, n); }

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zkmi_diag_group_mul_each_dev(int curve, int group, const void* d_points, const void* d_scalars_normal, void* d_out, size_t n) {
    ZK_TRY(require_ctx());
    if ((curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) || (group != 1 && group != 2)) return fail(ZKMI_ERR_INVALID, "group mul each: unknown curve or group");
    if (group != 1) return fail(ZKMI_ERR_UNSUPPORTED, "group mul each: G1 only (G2 runs the general kernel)");
    if (pipeline_busy()) return fail(ZKMI_ERR_INVALID, "group mul each: a pipeline slot holds work in flight (collect it first)");
    if (!n) return ZKMI_OK;
    if (!d_points || !d_scalars_normal || !d_out) return fail(ZKMI_ERR_INVALID, "group mul each: null buffer");
    if (n >= (1ull << 31)) return fail(ZKMI_ERR_UNSUPPORTED, "group mul each: at most 2^31 - 1 points");
    return mul_each_dispatch(curve, d_points, d_scalars_normal, d_out, n);
}
int zkmi_diag_set_ptau_slice(size_t points) {
    g_ptau_slice = points ? points : PTAU_SLICE_DEFAULT;
    return ZKMI_OK;
}

int zkmi_ptau_contribute_section(int curve, int group, zkmi_pages in, size_t n, const uint8_t* first, const uint8_t* inc, uint8_t* const* lem_ptr, const size_t* lem_len,
                                 int n_lem_pages, uint8_t* const* c_ptr, const size_t* c_len, int n_c_pages, uint8_t* const* u_ptr, const size_t* u_len, int n_u_pages) {
    ZK_TRY(require_ctx());
    if ((curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) || (group != 1 && group != 2)) return fail(ZKMI_ERR_INVALID, "ptau_contribute_section: unknown curve or group");
    if (!first || !inc) return fail(ZKMI_ERR_INVALID, "ptau_contribute_section: null argument");
    if (pipeline_busy()) return fail(ZKMI_ERR_INVALID, "ptau_contribute_section: a pipeline slot holds work in flight (collect it first)");
    if (!n) return ZKMI_OK;
    if (n >= (1ull << 31)) return fail(ZKMI_ERR_UNSUPPORTED, "ptau_contribute_section: at most 2^31 - 1 points");
    const size_t sG = (size_t)2 * group * n8q_of(curve), bytes = n * sG;
    if (!in.ptr || !in.len) return fail(ZKMI_ERR_INVALID, "ptau_contribute_section: null argument");
    if (pages_bytes(in) != bytes) return fail(ZKMI_ERR_INVALID, "ptau_contribute_section: the input pages do not hold n points");
    ZK_TRY(pages_check("LEM output", lem_ptr, lem_len, n_lem_pages, bytes));
    ZK_TRY(pages_check("C output", c_ptr, c_len, n_c_pages, bytes / 2));
    ZK_TRY(pages_check("U output", u_ptr, u_len, n_u_pages, bytes));
    DevMem dm("ptau_contribute_section");
    uint8_t *d_in, *d_lem, *d_form;
    ZK_TRY(dm.get(bytes, (void**)&d_in));
    ZK_TRY(dm.get(bytes, (void**)&d_lem));
    ZK_TRY(dm.get(bytes, (void**)&d_form));
    ZK_TRY(upload_pages(in, bytes, d_in));
    if (group == 1) ZK_TRY(contribute_g1(curve, d_in, d_lem, n, first, inc));
    else ZK_TRY(zkmi_group_batch_apply_key_dev(curve, 2, d_in, d_lem, n, first, inc));
    ZK_TRY(download_pages(d_lem, bytes, lem_ptr, lem_len, n_lem_pages));
    ZK_TRY(zkmi_group_convert_dev(curve, group, ZKMI_CONV_LEM_TO_C, d_lem, d_form, n));
    ZK_TRY(download_pages(d_form, bytes / 2, c_ptr, c_len, n_c_pages));
    ZK_TRY(zkmi_group_convert_dev(curve, group, ZKMI_CONV_LEM_TO_U, d_lem, d_form, n));
    return download_pages(d_form, bytes, u_ptr, u_len, n_u_pages);
}

int zkmi_blake2b512_partial(const uint8_t* const* chunks, const size_t* lens, int n, uint8_t* partial216) {
    if (n < 0 || (n && (!chunks || !lens)) || !partial216) return fail(ZKMI_ERR_INVALID, "blake2b512_partial: null argument");
    for (int i = 0; i < n; i++) if (lens[i] && !chunks[i]) return fail(ZKMI_ERR_INVALID, "blake2b512_partial: null argument");
    ptau::Blake2b512 hs;
    for (int i = 0; i < n; i++) hs.update_call(chunks[i], lens[i]);
    hs.partial(partial216);
    return ZKMI_OK;
}

}  // extern "C"
