// snarkjs_amd/csrc/plonk_setup.hip — host driver + C-ABI of the PLONK setup (src/plonk_setup.js) on the device.
//
// Host side, one serial pass over the r1cs constraint section: processConstraints (:143-302) lowers every constraint to PLONK rows. The pass is
// serial because reduceCoefs numbers the internal signals as it goes (plonkNVars++); it also notes, per position of the permutation, which
// position visited the same signal last (writeSigma's lastAparence / firstPos, :354-422), so that the device fills sigma by one gather.
// Device side: the selector columns, the permutation, the Lagrange polynomials, writeP4 (:326-333) for all of them through the library's own
// transforms, and the eight commitments over one resident table of the ceremony's Lagrange points.
#include <string.h>
#include <algorithm>
#include <chrono>
#include <vector>
#include "host_field.hpp"
#include "plonk_setup.cuh"
#include "setup_common.hpp"
#include "zkmi_common.hpp"

namespace zkmi {

namespace {

typedef host::HField<4> HF;
typedef host::HFp<4> E;

struct Lowered {
    uint32_t n_vars = 0;                          // plonkNVars
    std::vector<uint32_t> add_sig;                // 2 per addition
    std::vector<E> add_coef;                      // 2 per addition
    std::vector<uint32_t> map[3];
    std::vector<E> sel[5];                        // Qm, Ql, Qr, Qo, Qc
    uint32_t rows() const { return (uint32_t)map[0].size(); }
};

// cirPower of plonk_setup.js:74-75
int circuit_power(uint32_t rows) {
    const int p = ref_log2(rows - 1) + 1;
    return p < 3 ? 3 : p;
}

struct Lowering {
    const HF F;
    Lowered& L;
    const E zero, one;
    std::vector<Term> cs;                         // reduceCoefs' queue (shift from `head`, push at the back)
    Lowering(const HF& f, Lowered& l) : F(f), L(l), zero(f.zero()), one(f.One()) {}

    int row(uint32_t sl, uint32_t sr, uint32_t so, const E& qm, const E& ql, const E& qr, const E& qo, const E& qc) {
        if (L.map[0].size() >= 0xfffffff0u) return fail(ZKMI_ERR_UNSUPPORTED, "plonk_setup: more than 2^32 PLONK constraints");
        L.map[0].push_back(sl); L.map[1].push_back(sr); L.map[2].push_back(so);
        L.sel[0].push_back(qm); L.sel[1].push_back(ql); L.sel[2].push_back(qr); L.sel[3].push_back(qo); L.sel[4].push_back(qc);
        return ZKMI_OK;
    }
    // reduceCoefs (:175-218). Coefficients are byte arrays there, so `!= 0n` is always true: zero coefficients stay. It folds from the FRONT:
    // two entries leave, the new internal signal enters at the back with coefficient one.
    struct Reduced { E k; uint32_t s[3]; E c[3]; };
    int reduce(const Lc& lc, size_t max_c, Reduced& out) {
        out.k = zero;
        cs.clear();
        for (const Term& t : lc) { if (t.s == 0) out.k = t.c; else cs.push_back(t); }
        size_t head = 0;
        while (cs.size() - head > max_c) {
            const Term c1 = cs[head], c2 = cs[head + 1];
            head += 2;
            if (L.n_vars == 0xffffffffu) return fail(ZKMI_ERR_UNSUPPORTED, "plonk_setup: more than 2^32 signals");
            const uint32_t so = L.n_vars++;
            ZK_TRY(row(c1.s, c2.s, so, zero, F.neg(c1.c), F.neg(c2.c), one, zero));
            L.add_sig.push_back(c1.s); L.add_sig.push_back(c2.s);
            L.add_coef.push_back(c1.c); L.add_coef.push_back(c2.c);
            cs.push_back(Term{so, one});
        }
        for (size_t i = 0; i < max_c; i++) {
            if (head + i < cs.size()) { out.s[i] = cs[head + i].s; out.c[i] = cs[head + i].c; }
            else { out.s[i] = 0; out.c[i] = zero; }
        }
        return ZKMI_OK;
    }
    int sum(const Lc& lc) {                       // addConstraintSum (:220-231)
        Reduced C;
        ZK_TRY(reduce(lc, 3, C));
        return row(C.s[0], C.s[1], C.s[2], zero, C.c[0], C.c[1], C.c[2], C.k);
    }
    int mul(const Lc& a, const Lc& b, const Lc& c) {          // addConstraintMul (:233-248)
        Reduced A, B, C;
        ZK_TRY(reduce(a, 1, A));
        ZK_TRY(reduce(b, 1, B));
        ZK_TRY(reduce(c, 1, C));
        return row(A.s[0], B.s[0], C.s[0], F.mul(A.c[0], B.c[0]), F.mul(A.c[0], B.k), F.mul(A.k, B.c[0]), F.neg(C.c[0]), F.sub(F.mul(A.k, B.k), C.k));
    }
    // join (:152-173): k * lc1 - lc2, keys ascending; normalize deletes nothing (a byte array never equals 0n)
    void join(const Lc& lc1, const E& k, const Lc& lc2, Lc& res) {
        res.clear();
        size_t i = 0, j = 0;
        while (i < lc1.size() || j < lc2.size()) {
            if (j == lc2.size() || (i < lc1.size() && lc1[i].s < lc2[j].s)) { res.push_back(Term{lc1[i].s, F.mul(k, lc1[i].c)}); i++; }
            else if (i == lc1.size() || lc2[j].s < lc1[i].s) { res.push_back(Term{lc2[j].s, F.neg(lc2[j].c)}); j++; }
            else { res.push_back(Term{lc1[i].s, F.add(F.mul(k, lc1[i].c), F.neg(lc2[j].c))}); i++; j++; }
        }
    }
    // getLinearCombinationType (:250-266): 2 = has a signal other than 0 (a number there), 1 = "k", 0 = "0". `k != Fr.zero` compares identities,
    // so a combination whose only key is signal 0 is "k" whatever its coefficient.
    static int type_of(const Lc& lc) {
        for (const Term& t : lc) if (t.s != 0) return 2;
        return lc.empty() ? 0 : 1;
    }
    Lc joined;
    int process(const Lc& a, const Lc& b, const Lc& c) {       // :268-283
        const int ta = type_of(a), tb = type_of(b);
        if (ta == 0 || tb == 0) return sum(c);
        if (ta == 1) { join(b, a[0].c, c, joined); return sum(joined); }
        if (tb == 1) { join(a, b[0].c, c, joined); return sum(joined); }
        return mul(a, b, c);
    }
};

double g_psetup_ms[4] = {0, 0, 0, 0};             // lowering (host), sigma, P4, commitments: wall time of the last calls

template <class FrC> int lower(zkmi_pages constraints, uint32_t n_constraints, uint32_t n_vars, uint32_t n_public, Lowered& L) {
    const auto t0 = std::chrono::steady_clock::now();
    const HF F = HF::from_cfg<FrC>();
    // Deliberate deviation, the same as zkmi_groth16_setup_coeffs': the reference's reader checks neither nVars against nPublic nor a signal id
    // against nVars (its sparse arrays simply grow) and writes a key for such a file. No r1cs compiler emits one (signal 0 is the constant, so
    // nVars >= nPublic + 1), and here an id beyond plonkNVars would index past `last` / `first` in predecessors(): both are refused.
    if (n_vars <= n_public) return fail(ZKMI_ERR_INVALID, "plonk_setup: nVars must exceed nPublic");
    L.n_vars = n_vars;
    Lowering lw(F, L);
    for (uint32_t s = 1; s <= n_public; s++) ZK_TRY(lw.row(s, 0, 0, lw.zero, lw.one, lw.zero, lw.zero, lw.zero));      // the binding rows (:285-296)
    PageReader rd(constraints);
    Lc lc[3];
    std::vector<Term> raw;
    for (uint32_t c = 0; c < n_constraints; c++) {
        for (int k = 0; k < 3; k++) ZK_TRY(read_lc(rd, F, n_vars, raw, lc[k], "plonk_setup"));
        ZK_TRY(lw.process(lc[0], lc[1], lc[2]));
    }
    if (L.rows() == 0) return fail(ZKMI_ERR_INVALID, "plonk_setup: a circuit without constraints and without public signals");
    g_psetup_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ZKMI_OK;
}

int lower_any(int curve, zkmi_pages constraints, uint32_t n_constraints, uint32_t n_vars, uint32_t n_public, Lowered& L) {
    if (curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) return fail(ZKMI_ERR_INVALID, "plonk_setup: unknown curve");
    return curve == ZKMI_CURVE_BN128 ? lower<Bn254Fr>(constraints, n_constraints, n_vars, n_public, L) : lower<Bls12381Fr>(constraints, n_constraints, n_vars, n_public, L);
}

// writeSigma's bookkeeping (:354-422) turned into one index per position: visit order is row by row, columns a, b, c; padding rows hold signal 0
void predecessors(const Lowered& L, uint32_t domain, uint32_t* pred) {
    constexpr uint32_t NONE = 0xffffffffu;
    std::vector<uint32_t> last(L.n_vars, NONE), first(L.n_vars, NONE);
    const uint32_t rows = L.rows();
    for (uint32_t i = 0; i < domain; i++)
        for (uint32_t col = 0; col < 3; col++) {
            const uint32_t s = i < rows ? L.map[col][i] : 0u, p = col * domain + i;
            if (last[s] == NONE) first[s] = p; else pred[p] = last[s];
            last[s] = p;
        }
    for (uint32_t s = 0; s < L.n_vars; s++) if (first[s] != NONE) pred[first[s]] = last[s];     // a signal that never occurs: the reference's "Variable not used"
}

inline double ms_since(const std::chrono::steady_clock::time_point& t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

struct TableGuard {                               // the resident window table of one call
    uint64_t h = 0;
    ~TableGuard() { if (h) (void)zkmi_msm_table_release(h); }
};

template <class FqC, class FrC> int setup_run(const zkmi_plonk_setup_in& in, const zkmi_plonk_setup_out& out) {
    constexpr size_t sG1 = 2 * FqC::N * 4, sJ = 3 * FqC::N * 4;
    constexpr int W = FrC::N;
    Ctx& cx = ctx();
    hipStream_t st = cx.stream;
    const HF F = HF::from_cfg<FrC>();
    const uint32_t D = in.domain_size, rows = in.n_constraints;
    const size_t dom = D, n_poly = std::max<uint32_t>(in.n_public, 1u);
    const unsigned lg = (unsigned)ref_log2(D);
    if (out.q_len != 5 * dom * 32 || out.sigma_len != 15 * dom * 32 || out.lagrange_len != n_poly * 5 * dom * 32 || out.commitments_len != 8 * sG1)
        return fail(ZKMI_ERR_INVALID, "plonk_setup: an output buffer does not have the length of its section");
    for (int c = 0; c < 5; c++) if (!out.q[c]) return fail(ZKMI_ERR_INVALID, "plonk_setup: null output buffer");
    if (!out.sigma || !out.lagrange || !out.commitments || !in.selectors || !in.pred) return fail(ZKMI_ERR_INVALID, "plonk_setup: null buffer");
    if (pages_bytes(in.lagrange_g1) != dom * sG1) return fail(ZKMI_ERR_INVALID, "plonk_setup: the Lagrange slice does not hold domainSize points");
    for (size_t p = 0; p < 3 * dom; p++) if (in.pred[p] >= 3 * dom) return fail(ZKMI_ERR_INVALID, "plonk_setup: a predecessor index lies beyond the permutation");

    // getK1K2 (:484-504) never advances: Fr.add is called without an assignment, so it returns k1 = 2 and k2 = 3 or does not return at all
    // (2 and 3 lie outside every subgroup of 2^k elements on both curves, so it returns)
    E w, firsts[3] = {F.One(), F.from_u64(2), F.from_u64(3)};
    ZK_TRY(zkmi_fr_root(in.curve, lg, (uint8_t*)w.v));
    const E w_inv = F.inv(w), n_inv = F.inv(F.from_u64(D));
    Fp<FrC> one_dev;
    for (int i = 0; i < W; i++) one_dev.l[i] = FrC::one(i);

    DevMem dm("plonk_setup");
    uint32_t *d_sel, *d_pred, *d_ones, *d_ident, *d_cols, *d_sec, *d_lag, *d_pts;
    ZK_TRY(dm.get((size_t)5 * rows * 32, (void**)&d_sel));
    ZK_TRY(dm.get(3 * dom * 4, (void**)&d_pred));
    ZK_TRY(dm.get(dom * 32, (void**)&d_ones));
    ZK_TRY(dm.get(3 * dom * 32, (void**)&d_ident));
    ZK_TRY(dm.get(8 * dom * 32, (void**)&d_cols));                       // Qm Ql Qr Qo Qc S1 S2 S3: the evaluations the commitments take
    ZK_TRY(dm.get(8 * 5 * dom * 32, (void**)&d_sec));                    // sections 7 .. 11 and the three parts of section 12: n coefficients, 4n evaluations each
    ZK_TRY(dm.get(n_poly * 5 * dom * 32, (void**)&d_lag));               // section 13
    ZK_TRY(dm.get(dom * sG1, (void**)&d_pts));
    ZK_HIP(hipMemcpyAsync(d_sel, in.selectors, (size_t)5 * rows * 32, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_pred, in.pred, 3 * dom * 4, hipMemcpyHostToDevice, st));
    ZK_TRY(upload_pages(in.lagrange_g1, dom * sG1, d_pts));
    ZK_HIP(hipStreamSynchronize(st));
    const auto blocks = [](uint64_t n) { return dim3((unsigned)((n + 255) / 256)); };

    // ---- selectors and sigma
    auto t0 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL((k_psetup_pad<FrC>), blocks(5 * dom), dim3(256), 0, st, d_sel, d_cols, rows, D);
    hipLaunchKernelGGL((k_psetup_fill<FrC>), blocks(dom), dim3(256), 0, st, d_ones, (uint64_t)dom, one_dev);
    ZK_HIP(hipGetLastError());
    for (int col = 0; col < 3; col++) ZK_TRY(zkmi_fr_batch_apply_key_dev(in.curve, d_ones, d_ident + (size_t)col * dom * W, dom, (const uint8_t*)firsts[col].v, (const uint8_t*)w.v));
    hipLaunchKernelGGL((k_psetup_sigma<FrC>), blocks(3 * dom), dim3(256), 0, st, d_ident, d_pred, d_cols + 5 * dom * W, (uint64_t)(3 * dom));
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(st));
    g_psetup_ms[1] = ms_since(t0);

    // ---- writeP4 for the eight columns and the Lagrange polynomials
    t0 = std::chrono::steady_clock::now();
    for (int c = 0; c < 8; c++) {
        uint32_t* sec = d_sec + (size_t)c * 5 * dom * W;
        ZK_TRY(zkmi_ntt_dev(in.curve, d_cols + (size_t)c * dom * W, sec, lg, 1, nullptr, nullptr));
        ZK_TRY(zkmi_ntt_padded_dev(in.curve, sec, dom, sec + dom * W, lg + 2, 0));
    }
    // d_ident is free again: its first column becomes the table w^(-e) / n
    ZK_TRY(zkmi_fr_batch_apply_key_dev(in.curve, d_ones, d_ident, dom, (const uint8_t*)n_inv.v, (const uint8_t*)w_inv.v));
    hipLaunchKernelGGL((k_psetup_lagrange<FrC>), blocks(n_poly * dom), dim3(256), 0, st, d_ident, d_lag, (uint32_t)n_poly, D);
    ZK_HIP(hipGetLastError());
    for (size_t i = 0; i < n_poly; i++) {
        uint32_t* rec = d_lag + i * 5 * dom * W;
        ZK_TRY(zkmi_ntt_padded_dev(in.curve, rec, dom, rec + dom * W, lg + 2, 0));
    }
    ZK_HIP(hipStreamSynchronize(st));
    g_psetup_ms[2] = ms_since(t0);

    // ---- the eight commitments over one resident table
    t0 = std::chrono::steady_clock::now();
    uint8_t jac[8 * sJ];
    {
        TableGuard tab;
        ZK_TRY(zkmi_msm_table_build(in.curve, 1, d_pts, dom, &tab.h));
        for (int half = 0; half < 2; half++) {
            const void* polys[4];
            size_t ks[4];
            for (int k = 0; k < 4; k++) { polys[k] = d_cols + (size_t)(4 * half + k) * dom * W; ks[k] = dom; }
            ZK_TRY(zkmi_msm_table_multi_enqueue_mont_dev(tab.h, polys, ks, 4));
            ZK_TRY(zkmi_msm_table_multi_collect(tab.h, 4, jac + (size_t)half * 4 * sJ));
        }
    }
    for (int c = 0; c < 8; c++) ZK_TRY(zkmi_to_affine(in.curve, 1, jac + c * sJ, out.commitments + c * sG1));
    g_psetup_ms[3] = ms_since(t0);

    for (int c = 0; c < 5; c++) ZK_HIP(hipMemcpyAsync(out.q[c], d_sec + (size_t)c * 5 * dom * W, 5 * dom * 32, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(out.sigma, d_sec + (size_t)5 * 5 * dom * W, 15 * dom * 32, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(out.lagrange, d_lag, n_poly * 5 * dom * 32, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
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
    if (!counts4) return fail(ZKMI_ERR_INVALID, "plonk_setup_lower_len: null result");
    Lowered L;
    ZK_TRY(lower_any(curve, constraints, n_constraints, n_vars, n_public, L));
    counts4[0] = L.n_vars; counts4[1] = (uint32_t)(L.add_sig.size() / 2); counts4[2] = L.rows();
    const int power = circuit_power(L.rows());
    counts4[3] = power < 32 ? 1u << power : 0u;
    return ZKMI_OK;
}

int zkmi_plonk_setup_lower(int curve, zkmi_pages constraints, uint32_t n_constraints, uint32_t n_vars, uint32_t n_public, const zkmi_plonk_lowered* out) {
    if (!out || !out->map_a || !out->map_b || !out->map_c || !out->selectors || !out->pred || (out->n_additions && !out->additions))
        return fail(ZKMI_ERR_INVALID, "plonk_setup_lower: null buffer");
    Lowered L;
    ZK_TRY(lower_any(curve, constraints, n_constraints, n_vars, n_public, L));
    const uint32_t rows = L.rows(), n_add = (uint32_t)(L.add_sig.size() / 2);
    const int power = circuit_power(rows);
    if (out->plonk_n_vars != L.n_vars || out->n_additions != n_add || out->n_constraints != rows || power >= 31 || out->domain_size != 1u << power)
        return fail(ZKMI_ERR_INVALID, "plonk_setup_lower: the counts do not match the constraints (zkmi_plonk_setup_lower_len)");
    for (uint32_t i = 0; i < n_add; i++) {
        uint8_t* rec = out->additions + (size_t)i * 72;
        memcpy(rec, &L.add_sig[2 * i], 8);
        memcpy(rec + 8, L.add_coef[2 * i].v, 32);
        memcpy(rec + 40, L.add_coef[2 * i + 1].v, 32);
    }
    uint32_t* const maps[3] = {out->map_a, out->map_b, out->map_c};
    for (int k = 0; k < 3; k++) memcpy(maps[k], L.map[k].data(), (size_t)rows * 4);
    for (int k = 0; k < 5; k++) memcpy(out->selectors + (size_t)k * rows * 32, L.sel[k].data(), (size_t)rows * 32);
    predecessors(L, out->domain_size, out->pred);
    return ZKMI_OK;
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
