// snarkjs_amd/csrc/plonk_setup.hip — host driver + C-ABI of the PLONK setup (src/plonk_setup.js) on the device.
//
// Host side, one serial pass over the r1cs constraint section: processConstraints (:143-302) lowers every constraint to PLONK rows. The pass is
// serial because reduceCoefs numbers the internal signals as it goes (plonkNVars++); it also notes, per position of the permutation, which
// position visited the same signal last (writeSigma's lastAparence / firstPos, :354-422), so that the device fills sigma by one gather.
// Device side: the selector columns, the permutation, the Lagrange polynomials, writeP4 (:326-333) for all of them through the library's own
// transforms, and the eight commitments over one resident table of the ceremony's Lagrange points.
// The lowering and the device steps up to writeP4 are gate_setup.hpp's, shared with fflonk_setup.hip; here are PLONK's rules for them, its curve
// policy, its checks, the commitments and the entry points.
#include <chrono>
#include "gate_setup.hpp"
#include "zkmi_common.hpp"

namespace zkmi {

namespace {

// plonk_setup.js. drop_zeros: normalize (:152-173) compares a byte array with 0n and deletes nothing. free_rows: cirPower is log2(rows - 1) + 1
// (:74-75) and writeSigma (:354-422) walks every row of the domain. sel_col: writeQMap (:313-318) and sections 7 - 11 are Qm Ql Qr Qo Qc.
const GateRules PLONK_RULES = {"plonk_setup", false, 0, {1, 2, 0, 3, 4}};

double g_psetup_ms[4] = {0, 0, 0, 0};             // lowering (host), sigma, P4, commitments: wall time of the last calls

// both curves: the reference's setup is the same program on either
int field_of(int curve, HF& F) {
    if (curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) return fail(ZKMI_ERR_INVALID, "plonk_setup: unknown curve");
    F = curve == ZKMI_CURVE_BN128 ? HF::from_cfg<Bn254Fr>() : HF::from_cfg<Bls12381Fr>();
    return ZKMI_OK;
}

struct TableGuard {                               // the resident window table of one call
    uint64_t h = 0;
    ~TableGuard() { if (h) (void)zkmi_msm_table_release(h); }
};

template <class FqC, class FrC> int setup_run(const zkmi_plonk_setup_in& in, const zkmi_plonk_setup_out& out) {
    constexpr size_t sG1 = 2 * FqC::N * 4, sJ = 3 * FqC::N * 4;
    constexpr int W = FrC::N;
    const size_t dom = in.domain_size;
    if (out.commitments_len != 8 * sG1) return fail(ZKMI_ERR_INVALID, "plonk_setup: an output buffer does not have the length of its section");
    if (!out.commitments) return fail(ZKMI_ERR_INVALID, "plonk_setup: null buffer");
    GateDevice<FqC, FrC> dev("plonk_setup");
    ZK_TRY(dev.run(in.curve, in.n_public, in.n_constraints, in.domain_size, in.selectors, in.pred, out.q, out.q_len, out.sigma, out.sigma_len, out.lagrange,
                   out.lagrange_len, in.lagrange_g1, dom, "the Lagrange slice does not hold domainSize points", g_psetup_ms));

    // ---- the eight commitments over one resident table
    const auto t0 = std::chrono::steady_clock::now();
    uint8_t jac[8 * sJ];
    {
        TableGuard tab;
        ZK_TRY(zkmi_msm_table_build(in.curve, 1, dev.d_pts, dom, &tab.h));
        for (int half = 0; half < 2; half++) {
            const void* polys[4];
            size_t ks[4];
            for (int k = 0; k < 4; k++) { polys[k] = dev.d_cols + (size_t)(4 * half + k) * dom * W; ks[k] = dom; }
            ZK_TRY(zkmi_msm_table_multi_enqueue_mont_dev(tab.h, polys, ks, 4));
            ZK_TRY(zkmi_msm_table_multi_collect(tab.h, 4, jac + (size_t)half * 4 * sJ));
        }
    }
    for (int c = 0; c < 8; c++) ZK_TRY(zkmi_to_affine(in.curve, 1, jac + c * sJ, out.commitments + c * sG1));
    g_psetup_ms[3] = ms_since(t0);

    ZK_TRY(dev.download(out.q, out.sigma, out.lagrange));
    ZK_HIP(hipStreamSynchronize(ctx().stream));
    ZK_HIP(hipGetLastError());
    return ZKMI_OK;
}

int setup_check(const zkmi_plonk_setup_in* in) {
    if (!in) return fail(ZKMI_ERR_INVALID, "plonk_setup: null descriptor");
    if (in->curve != ZKMI_CURVE_BN128 && in->curve != ZKMI_CURVE_BLS12381) return fail(ZKMI_ERR_INVALID, "plonk_setup: unknown curve");
    const uint64_t d = in->domain_size;
    if (d < 8 || (d & (d - 1))) return fail(ZKMI_ERR_INVALID, "plonk_setup: domainSize must be a power of two, at least 8");
    if (d > (1ull << 26)) return fail(ZKMI_ERR_UNSUPPORTED, "plonk_setup: domains above 2^26 are not supported (the 4n evaluations must fit the two-adicity of both curves)");
    if (in->n_constraints == 0 || in->n_constraints > d) return fail(ZKMI_ERR_INVALID, "plonk_setup: the PLONK constraints do not fit domainSize");
    if (in->n_public > in->n_constraints) return fail(ZKMI_ERR_INVALID, "plonk_setup: more public signals than constraints");
    return ZKMI_OK;
}

}  // namespace

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zkmi_plonk_setup_lower_len(int curve, zkmi_pages constraints, uint32_t n_constraints, uint32_t n_vars, uint32_t n_public, uint32_t* counts4) {
    HF F;
    ZK_TRY(field_of(curve, F));
    return lower_len_body(PLONK_RULES, F, constraints, n_constraints, n_vars, n_public, counts4, g_psetup_ms[0]);
}

int zkmi_plonk_setup_lower(int curve, zkmi_pages constraints, uint32_t n_constraints, uint32_t n_vars, uint32_t n_public, const zkmi_plonk_lowered* out) {
    HF F;
    ZK_TRY(field_of(curve, F));
    return lower_body(PLONK_RULES, F, constraints, n_constraints, n_vars, n_public, out, g_psetup_ms[0]);
}

int zkmi_plonk_setup(const zkmi_plonk_setup_in* in, const zkmi_plonk_setup_out* out) {
    ZK_TRY(require_ctx());
    ZK_TRY(setup_check(in));
    if (!out) return fail(ZKMI_ERR_INVALID, "plonk_setup: null output descriptor");
    if (pipeline_busy()) return fail(ZKMI_ERR_INVALID, "plonk_setup: a pipeline slot holds work in flight (collect it first)");
    return in->curve == ZKMI_CURVE_BN128 ? setup_run<Bn254Fq, Bn254Fr>(*in, *out) : setup_run<Bls12381Fq, Bls12381Fr>(*in, *out);
}

int zkmi_plonk_setup_phase_ms(double* out4) {
    if (!out4) return fail(ZKMI_ERR_INVALID, "plonk_setup_phase_ms: null result");
    for (int i = 0; i < 4; i++) out4[i] = g_psetup_ms[i];
    return ZKMI_OK;
}

}  // extern "C"
