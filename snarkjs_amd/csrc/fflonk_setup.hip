// snarkjs_amd/csrc/fflonk_setup.hip — host driver + C-ABI of the FFLONK setup (src/fflonk_setup.js) on the device.
//
// Host side, one serial pass over the r1cs constraint section: computeFFConstraints (:160-209) through src/r1cs_constraint_processor.js lowers every
// constraint to rows [a, b, c, ql, qr, qm, qo, qc]. The pass also notes, per position of the permutation, which position visited the same signal last
// (writeSigma :340-415), so that k_psetup_sigma serves unchanged.
// Device side: the kernels of plonk_setup.cuh and the library's transforms for sections 7 - 15, k_fsetup_c0 for section 17 and the MSM scalars, one MSM.
// The lowering and the device steps up to writeP4 are gate_setup.hpp's, shared with plonk_setup.hip; here are FFLONK's rules for them (FFLONK_RULES:
// where it is NOT the lowering of PLONK), its curve policy, its checks, C0 with its commitment and the entry points.
#include <chrono>
#include "fflonk_setup.cuh"
#include "gate_setup.hpp"
#include "zkmi_common.hpp"

namespace zkmi {

namespace {

// fflonk_setup.js with r1cs_constraint_processor.js. drop_zeros: normalizeLinearCombination (r1cs_constraint_processor.js:86-93) asks Fr.isZero, which
// reads the Montgomery bytes, so zero coefficients leave a combination before it is classified (:32-51) and after a join (:95-116). free_rows: cirPower
// is log2(rows + 1) + 1 (fflonk_setup.js:112), two rows of the domain stay free for the blinding coefficients, and writeSigma (:356-359) leaves them the
// identity. sel_col: the rows are [.., ql, qr, qm, qo, qc] and sections 7 - 11 are QL QR QM QO QC.
const GateRules FFLONK_RULES = {"fflonk_setup", true, 2, {0, 1, 2, 3, 4}};

double g_fsetup_ms[4] = {0, 0, 0, 0};             // lowering (host), sigma, P4, C0 and its commitment: wall time of the last calls

// The reference's fflonk.setup writes BN254's w3 and wr whatever the curve: a BLS12-381 key of its making proves nothing, and none is made here
int curve_check(int curve) {
    if (curve == ZKMI_CURVE_BLS12381) return fail(ZKMI_ERR_UNSUPPORTED, "fflonk_setup: BN254 only (the reference's setup writes BN254's roots into a BLS12-381 key)");
    if (curve != ZKMI_CURVE_BN128) return fail(ZKMI_ERR_INVALID, "fflonk_setup: unknown curve");
    return ZKMI_OK;
}

template <class FqC, class FrC> int setup_run(const zkmi_fflonk_setup_in& in, const zkmi_fflonk_setup_out& out) {
    constexpr size_t sG1 = 2 * FqC::N * 4, sJ = 3 * FqC::N * 4;
    const uint32_t D = in.domain_size;
    const size_t dom = D;
    hipStream_t st = ctx().stream;
    // deg C0 < 8n holds by construction (eight polynomials of n coefficients): the lengths are all there is to check
    if (out.c0_len != 8 * dom * 32 || out.commitment_len != sG1) return fail(ZKMI_ERR_INVALID, "fflonk_setup: an output buffer does not have the length of its section");
    if (!out.c0 || !out.commitment) return fail(ZKMI_ERR_INVALID, "fflonk_setup: null buffer");
    GateDevice<FqC, FrC> dev("fflonk_setup");
    ZK_TRY(dev.run(in.curve, in.n_public, in.n_constraints, D, in.selectors, in.pred, out.q, out.q_len, out.sigma, out.sigma_len, out.lagrange, out.lagrange_len,
                   in.tau_g1, 8 * dom, "the tauG1 slice does not hold 8 * domainSize points", g_fsetup_ms));
    uint32_t *d_c0, *d_sc;
    ZK_TRY(dev.dm.get(8 * dom * 32, (void**)&d_c0));                     // section 17
    ZK_TRY(dev.dm.get(8 * dom * 32, (void**)&d_sc));                     // the same, canonical: the MSM's scalars

    // ---- C0 and its commitment: the bases are used once, so the plain MSM (one copy of the points) and no window table
    const auto t0 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL((k_fsetup_c0<FrC>), dim3((unsigned)((8 * dom + 255) / 256)), dim3(256), 0, st, dev.d_sec, d_c0, d_sc, D);
    ZK_HIP(hipGetLastError());
    uint8_t jac[sJ];
    ZK_TRY(zkmi_msm_dev(in.curve, 1, dev.d_pts, d_sc, 8 * dom, 32, jac));
    ZK_TRY(zkmi_to_affine(in.curve, 1, jac, out.commitment));
    g_fsetup_ms[3] = ms_since(t0);

    ZK_TRY(dev.download(out.q, out.sigma, out.lagrange));
    ZK_HIP(hipMemcpyAsync(out.c0, d_c0, 8 * dom * 32, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    return ZKMI_OK;
}

int setup_check(const zkmi_fflonk_setup_in* in) {
    if (!in) return fail(ZKMI_ERR_INVALID, "fflonk_setup: null descriptor");
    ZK_TRY(curve_check(in->curve));
    const uint64_t d = in->domain_size;
    if (d < 8 || (d & (d - 1))) return fail(ZKMI_ERR_INVALID, "fflonk_setup: domainSize must be a power of two, at least 8");
    if (d > (1ull << 26)) return fail(ZKMI_ERR_UNSUPPORTED, "fflonk_setup: domains above 2^26 are not supported (the 4n evaluations must fit the two-adicity of the field)");
    if (in->n_constraints == 0 || (uint64_t)in->n_constraints + 2 > d) return fail(ZKMI_ERR_INVALID, "fflonk_setup: the constraints and the two free rows do not fit domainSize");
    if (in->n_public > in->n_constraints) return fail(ZKMI_ERR_INVALID, "fflonk_setup: more public signals than constraints");
    return ZKMI_OK;
}

}  // namespace

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zkmi_fflonk_setup_lower_len(int curve, zkmi_pages constraints, uint32_t n_constraints, uint32_t n_vars, uint32_t n_public, uint32_t* counts4) {
    ZK_TRY(curve_check(curve));
    return lower_len_body(FFLONK_RULES, HF::from_cfg<Bn254Fr>(), constraints, n_constraints, n_vars, n_public, counts4, g_fsetup_ms[0]);
}

int zkmi_fflonk_setup_lower(int curve, zkmi_pages constraints, uint32_t n_constraints, uint32_t n_vars, uint32_t n_public, const zkmi_plonk_lowered* out) {
    ZK_TRY(curve_check(curve));
    return lower_body(FFLONK_RULES, HF::from_cfg<Bn254Fr>(), constraints, n_constraints, n_vars, n_public, out, g_fsetup_ms[0]);
}

int zkmi_fflonk_setup(const zkmi_fflonk_setup_in* in, const zkmi_fflonk_setup_out* out) {
    ZK_TRY(setup_check(in));
    ZK_TRY(require_ctx());
    if (!out) return fail(ZKMI_ERR_INVALID, "fflonk_setup: null output descriptor");
    if (pipeline_busy()) return fail(ZKMI_ERR_INVALID, "fflonk_setup: a pipeline slot holds work in flight (collect it first)");
    return setup_run<Bn254Fq, Bn254Fr>(*in, *out);
}

int zkmi_fflonk_setup_phase_ms(double* out4) {
    if (!out4) return fail(ZKMI_ERR_INVALID, "fflonk_setup_phase_ms: null result");
    for (int i = 0; i < 4; i++) out4[i] = g_fsetup_ms[i];
    return ZKMI_OK;
}

}  // extern "C"
