// snarkjs_amd/csrc/gate_setup.hpp — what the two gate setups (plonk_setup.hip: src/plonk_setup.js, fflonk_setup.hip: src/fflonk_setup.js with
// src/r1cs_constraint_processor.js) share: the serial lowering of the r1cs constraint section to rows [a, b, c, ql, qr, qm, qo, qc], the
// permutation's predecessor map, the bodies of the two lowering entry points, and the device steps up to the end of writeP4 with their downloads.
// What differs between the two protocols is the GateRules record, one constant per unit. Where a comment cites two places, the first is
// plonk_setup.js and the second is r1cs_constraint_processor.js (fflonk_setup.js where it says so).
#pragma once
#include <string.h>
#include <algorithm>
#include <chrono>
#include <string>
#include <vector>
#include "host_field.hpp"
#include "plonk_setup.cuh"
#include "setup_common.hpp"
#include "zkmi_common.hpp"

namespace zkmi {

namespace {                                       // internal to each of the two units, as setup_common.hpp is

typedef host::HField<4> HF;
typedef host::HFp<4> E;

struct GateRules {
    const char* who;                              // "plonk_setup" / "fflonk_setup": prefix of every error text
    bool drop_zeros;                              // normalizeLinearCombination really deletes zero coefficients, before classifying and after a join
    uint32_t free_rows;                           // rows at the top of the domain that keep the identity and count towards cirPower
    uint8_t sel_col[5];                           // where ql, qr, qm, qo, qc land among the five selector columns
};

struct Lowered {
    uint32_t n_vars = 0;                          // plonkNVars / settings.nVars: grows with every addition
    std::vector<uint32_t> add_sig;                // 2 per addition
    std::vector<E> add_coef;                      // 2 per addition
    std::vector<uint32_t> map[3];
    std::vector<E> sel[5];                        // the selector columns in the protocol's order (GateRules::sel_col)
    uint32_t rows() const { return (uint32_t)map[0].size(); }
};

// cirPower (plonk_setup.js:74-75, fflonk_setup.js:112)
inline int circuit_power(uint32_t rows, uint32_t free_rows) {
    const int p = ref_log2(rows + free_rows - 1) + 1;
    return p < 3 ? 3 : p;
}

struct Lowering {
    const GateRules& R;
    const HF F;
    Lowered& L;
    const E zero, one;
    std::vector<Term> cs;                         // reduceCoefs' queue (shift from `head`, push at the back)
    Lowering(const GateRules& r, const HF& f, Lowered& l) : R(r), F(f), L(l), zero(f.zero()), one(f.One()) {}

    int row(uint32_t a, uint32_t b, uint32_t c, const E& ql, const E& qr, const E& qm, const E& qo, const E& qc) {
        if (L.map[0].size() >= 0xfffffff0u) return fail(ZKMI_ERR_UNSUPPORTED, std::string(R.who) + ": more than 2^32 constraints");
        L.map[0].push_back(a); L.map[1].push_back(b); L.map[2].push_back(c);
        const E* const q[5] = {&ql, &qr, &qm, &qo, &qc};
        for (int k = 0; k < 5; k++) L.sel[R.sel_col[k]].push_back(*q[k]);
        return ZKMI_OK;
    }
    // normalizeLinearCombination. plonk_setup.js:152-173 compares a byte array with 0n, so it deletes nothing; r1cs_constraint_processor.js:86-93
    // asks Fr.isZero, which reads the Montgomery bytes, so zero coefficients DO leave (GateRules::drop_zeros)
    static void normalize(Lc& lc) {
        lc.erase(std::remove_if(lc.begin(), lc.end(), [](const Term& t) { return t.c.is_zero(); }), lc.end());
    }
    // getLinearCombinationType (:250-266, :53-84): 2 = has a signal other than 0 (a number there), 1 = "k", 0 = "0". `k != Fr.zero` compares
    // identities (the other file's `== 0n` compares a byte array and never fires), so a combination whose only key is signal 0 is "k" whatever its
    // coefficient.
    static int type_of(const Lc& lc) {
        for (const Term& t : lc) if (t.s != 0) return 2;
        return lc.empty() ? 0 : 1;
    }
    // reduceCoefs (:175-218, :118-160). Coefficients are byte arrays there, so `!= 0n` is always true: zero coefficients stay. It folds from the
    // FRONT: two entries leave, the new internal signal enters at the back with coefficient one.
    struct Reduced { E k; uint32_t s[3]; E c[3]; };
    int reduce(const Lc& lc, size_t max_c, Reduced& out) {
        out.k = zero;
        cs.clear();
        for (const Term& t : lc) { if (t.s == 0) out.k = t.c; else cs.push_back(t); }
        size_t head = 0;
        while (cs.size() - head > max_c) {
            const Term c1 = cs[head], c2 = cs[head + 1];
            head += 2;
            if (L.n_vars == 0xffffffffu) return fail(ZKMI_ERR_UNSUPPORTED, std::string(R.who) + ": more than 2^32 signals");
            const uint32_t so = L.n_vars++;
            ZK_TRY(row(c1.s, c2.s, so, F.neg(c1.c), F.neg(c2.c), zero, one, zero));
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
    int sum(const Lc& lc) {                       // addConstraintSum (:220-231), processR1csAdditionConstraint (:162-175)
        Reduced C;
        ZK_TRY(reduce(lc, 3, C));
        return row(C.s[0], C.s[1], C.s[2], C.c[0], C.c[1], zero, C.c[2], C.k);
    }
    int mul(const Lc& a, const Lc& b, const Lc& c) {          // addConstraintMul (:233-248), processR1csMultiplicationConstraint (:177-196)
        Reduced A, B, C;
        ZK_TRY(reduce(a, 1, A));
        ZK_TRY(reduce(b, 1, B));
        ZK_TRY(reduce(c, 1, C));
        return row(A.s[0], B.s[0], C.s[0], F.mul(A.c[0], B.k), F.mul(A.k, B.c[0]), F.mul(A.c[0], B.c[0]), F.neg(C.c[0]), F.sub(F.mul(A.k, B.k), C.k));
    }
    // join (:152-173), joinLinearCombinations (:95-116): k * lc1 - lc2, keys ascending; with drop_zeros the terms that cancel leave
    void join(const Lc& lc1, const E& k, const Lc& lc2, Lc& res) {
        res.clear();
        size_t i = 0, j = 0;
        while (i < lc1.size() || j < lc2.size()) {
            if (j == lc2.size() || (i < lc1.size() && lc1[i].s < lc2[j].s)) { res.push_back(Term{lc1[i].s, F.mul(k, lc1[i].c)}); i++; }
            else if (i == lc1.size() || lc2[j].s < lc1[i].s) { res.push_back(Term{lc2[j].s, F.neg(lc2[j].c)}); j++; }
            else { res.push_back(Term{lc1[i].s, F.add(F.mul(k, lc1[i].c), F.neg(lc2[j].c))}); i++; j++; }
        }
        if (R.drop_zeros) normalize(res);
    }
    Lc joined;
    int process(Lc& a, Lc& b, Lc& c) {            // :268-283, processR1csConstraint (:32-51)
        if (R.drop_zeros) { normalize(a); normalize(b); normalize(c); }
        const int ta = type_of(a), tb = type_of(b);
        if (ta == 0 || tb == 0) return sum(c);
        if (ta == 1) { join(b, a[0].c, c, joined); return sum(joined); }
        if (tb == 1) { join(a, b[0].c, c, joined); return sum(joined); }
        return mul(a, b, c);
    }
};

inline double ms_since(const std::chrono::steady_clock::time_point& t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// processConstraints (plonk_setup.js:143-302), computeFFConstraints (fflonk_setup.js:160-209); `ms` takes the wall time of the pass
inline int lower(const GateRules& R, const HF& F, zkmi_pages constraints, uint32_t n_constraints, uint32_t n_vars, uint32_t n_public, Lowered& L, double& ms) {
    const auto t0 = std::chrono::steady_clock::now();
    // Deliberate deviation, the same as zkmi_groth16_setup_coeffs': the reference's reader checks neither nVars against nPublic nor a signal id
    // against nVars (its sparse arrays simply grow) and writes a key for such a file. No r1cs compiler emits one (signal 0 is the constant, so
    // nVars >= nPublic + 1), and here an id beyond plonkNVars would index past `last` / `first` in predecessors(): both are refused.
    if (n_vars <= n_public) return fail(ZKMI_ERR_INVALID, std::string(R.who) + ": nVars must exceed nPublic");
    L.n_vars = n_vars;
    Lowering lw(R, F, L);
    // the binding rows (:285-296), getFFlonkConstantConstraint
    for (uint32_t s = 1; s <= n_public; s++) ZK_TRY(lw.row(s, 0, 0, lw.one, lw.zero, lw.zero, lw.zero, lw.zero));
    PageReader rd(constraints);
    Lc lc[3];
    std::vector<Term> raw;
    for (uint32_t c = 0; c < n_constraints; c++) {
        for (int k = 0; k < 3; k++) ZK_TRY(read_lc(rd, F, n_vars, raw, lc[k], R.who));
        ZK_TRY(lw.process(lc[0], lc[1], lc[2]));
    }
    if (L.rows() == 0) return fail(ZKMI_ERR_INVALID, std::string(R.who) + ": a circuit without constraints and without public signals");
    ms = ms_since(t0);
    return ZKMI_OK;
}

// writeSigma's bookkeeping (plonk_setup.js:354-422, fflonk_setup.js:340-415) turned into one index per position: visit order is row by row, columns
// a, b, c; the rows from the constraint count up hold signal 0; the last free_rows rows keep the identity and belong to no signal's cycle
inline void predecessors(const Lowered& L, uint32_t domain, uint32_t free_rows, uint32_t* pred) {
    constexpr uint32_t NONE = 0xffffffffu;
    std::vector<uint32_t> last(L.n_vars, NONE), first(L.n_vars, NONE);
    const uint32_t rows = L.rows();
    for (uint32_t i = 0; i < domain; i++)
        for (uint32_t col = 0; col < 3; col++) {
            const uint32_t p = col * domain + i;
            if (i >= domain - free_rows) { pred[p] = p; continue; }       // rows <= domain - free_rows (circuit_power)
            const uint32_t s = i < rows ? L.map[col][i] : 0u;
            if (last[s] == NONE) first[s] = p; else pred[p] = last[s];
            last[s] = p;
        }
    for (uint32_t s = 0; s < L.n_vars; s++) if (first[s] != NONE) pred[first[s]] = last[s];     // a signal that never occurs: the reference's "Variable not used"
}

// ---- the bodies of zkmi_*_setup_lower_len and zkmi_*_setup_lower, after the unit's curve policy has chosen the field
inline int lower_len_body(const GateRules& R, const HF& F, zkmi_pages constraints, uint32_t n_constraints, uint32_t n_vars, uint32_t n_public, uint32_t* counts4, double& ms) {
    if (!counts4) return fail(ZKMI_ERR_INVALID, std::string(R.who) + "_lower_len: null result");
    Lowered L;
    ZK_TRY(lower(R, F, constraints, n_constraints, n_vars, n_public, L, ms));
    counts4[0] = L.n_vars; counts4[1] = (uint32_t)(L.add_sig.size() / 2); counts4[2] = L.rows();
    const int power = circuit_power(L.rows(), R.free_rows);
    counts4[3] = power < 32 ? 1u << power : 0u;
    return ZKMI_OK;
}

inline int lower_body(const GateRules& R, const HF& F, zkmi_pages constraints, uint32_t n_constraints, uint32_t n_vars, uint32_t n_public, const zkmi_plonk_lowered* out, double& ms) {
    if (!out || !out->map_a || !out->map_b || !out->map_c || !out->selectors || !out->pred || (out->n_additions && !out->additions))
        return fail(ZKMI_ERR_INVALID, std::string(R.who) + "_lower: null buffer");
    Lowered L;
    ZK_TRY(lower(R, F, constraints, n_constraints, n_vars, n_public, L, ms));
    const uint32_t rows = L.rows(), n_add = (uint32_t)(L.add_sig.size() / 2);
    const int power = circuit_power(rows, R.free_rows);
    if (out->plonk_n_vars != L.n_vars || out->n_additions != n_add || out->n_constraints != rows || power >= 31 || out->domain_size != 1u << power)
        return fail(ZKMI_ERR_INVALID, std::string(R.who) + "_lower: the counts do not match the constraints (zkmi_" + R.who + "_lower_len)");
    for (uint32_t i = 0; i < n_add; i++) {
        uint8_t* rec = out->additions + (size_t)i * 72;
        memcpy(rec, &L.add_sig[2 * i], 8);
        memcpy(rec + 8, L.add_coef[2 * i].v, 32);
        memcpy(rec + 40, L.add_coef[2 * i + 1].v, 32);
    }
    uint32_t* const maps[3] = {out->map_a, out->map_b, out->map_c};
    for (int k = 0; k < 3; k++) memcpy(maps[k], L.map[k].data(), (size_t)rows * 4);
    for (int k = 0; k < 5; k++) memcpy(out->selectors + (size_t)k * rows * 32, L.sel[k].data(), (size_t)rows * 32);
    predecessors(L, out->domain_size, R.free_rows, out->pred);
    return ZKMI_OK;
}

// ---- the device steps of one setup call that both protocols take, on the active slot's stream: the selector columns and sigma, then writeP4
// (plonk_setup.js:326-333; Polynomial.fromEvaluations + Evaluations.fromPolynomial(4) in fflonk_setup.js) for the eight columns and the Lagrange
// polynomials. The unit's commitment step reads d_cols, d_sec and d_pts afterwards; the memory lives as long as this object.
template <class FqC, class FrC> struct GateDevice {
    static constexpr size_t sG1 = 2 * FqC::N * 4;
    static constexpr int W = FrC::N;
    DevMem dm;
    size_t dom = 0, n_poly = 0;
    uint32_t *d_cols = nullptr;                   // the five selector columns in the protocol's order, then S1 S2 S3: the evaluations on the domain
    uint32_t *d_sec = nullptr;                    // zkey sections 7 .. 11 and the three records of sigma: n coefficients, 4n evaluations each
    uint32_t *d_lag = nullptr;                    // the section of the Lagrange polynomials
    uint32_t *d_pts = nullptr;                    // the n_points ceremony points of the commitment step
    explicit GateDevice(const char* who) : dm(who) {}

    // check, allocate, upload, selectors + sigma (ms[1]), writeP4 + Lagrange (ms[2]). `points_text` is the refusal of a slice of another size.
    int run(int curve, uint32_t n_public, uint32_t rows, uint32_t D, const uint8_t* selectors, const uint32_t* pred, uint8_t* const* q, size_t q_len,
            const uint8_t* sigma, size_t sigma_len, const uint8_t* lagrange, size_t lagrange_len, const zkmi_pages& points, size_t n_points,
            const char* points_text, double* ms) {
        const std::string who = dm.who;
        hipStream_t st = ctx().stream;
        const HF F = HF::from_cfg<FrC>();
        dom = D; n_poly = std::max<uint32_t>(n_public, 1u);
        const unsigned lg = (unsigned)ref_log2(D);
        if (q_len != 5 * dom * 32 || sigma_len != 15 * dom * 32 || lagrange_len != n_poly * 5 * dom * 32)
            return fail(ZKMI_ERR_INVALID, who + ": an output buffer does not have the length of its section");
        for (int c = 0; c < 5; c++) if (!q[c]) return fail(ZKMI_ERR_INVALID, who + ": null output buffer");
        if (!sigma || !lagrange || !selectors || !pred) return fail(ZKMI_ERR_INVALID, who + ": null buffer");
        if (pages_bytes(points) != n_points * sG1) return fail(ZKMI_ERR_INVALID, who + ": " + points_text);
        for (size_t p = 0; p < 3 * dom; p++) if (pred[p] >= 3 * dom) return fail(ZKMI_ERR_INVALID, who + ": a predecessor index lies beyond the permutation");

        // getK1K2 (plonk_setup.js:484-504), computeK1K2 (fflonk_setup.js:513-532) never advance: Fr.add is called without an assignment, so they
        // return k1 = 2 and k2 = 3 or do not return at all (2 and 3 lie outside every subgroup of 2^k elements on both curves, so they return)
        E w, firsts[3] = {F.One(), F.from_u64(2), F.from_u64(3)};
        ZK_TRY(zkmi_fr_root(curve, lg, (uint8_t*)w.v));
        const E w_inv = F.inv(w), n_inv = F.inv(F.from_u64(D));
        Fp<FrC> one_dev;
        for (int i = 0; i < W; i++) one_dev.l[i] = FrC::one(i);

        uint32_t *d_sel, *d_pred, *d_ones, *d_ident;
        ZK_TRY(dm.get((size_t)5 * rows * 32, (void**)&d_sel));
        ZK_TRY(dm.get(3 * dom * 4, (void**)&d_pred));
        ZK_TRY(dm.get(dom * 32, (void**)&d_ones));
        ZK_TRY(dm.get(3 * dom * 32, (void**)&d_ident));
        ZK_TRY(dm.get(8 * dom * 32, (void**)&d_cols));
        ZK_TRY(dm.get(8 * 5 * dom * 32, (void**)&d_sec));
        ZK_TRY(dm.get(n_poly * 5 * dom * 32, (void**)&d_lag));
        ZK_TRY(dm.get(n_points * sG1, (void**)&d_pts));
        ZK_HIP(hipMemcpyAsync(d_sel, selectors, (size_t)5 * rows * 32, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemcpyAsync(d_pred, pred, 3 * dom * 4, hipMemcpyHostToDevice, st));
        ZK_TRY(upload_pages(points, n_points * sG1, d_pts));
        ZK_HIP(hipStreamSynchronize(st));
        const auto blocks = [](uint64_t n) { return dim3((unsigned)((n + 255) / 256)); };

        // ---- selectors and sigma
        auto t0 = std::chrono::steady_clock::now();
        hipLaunchKernelGGL((k_psetup_pad<FrC>), blocks(5 * dom), dim3(256), 0, st, d_sel, d_cols, rows, D);
        hipLaunchKernelGGL((k_psetup_fill<FrC>), blocks(dom), dim3(256), 0, st, d_ones, (uint64_t)dom, one_dev);
        ZK_HIP(hipGetLastError());
        for (int col = 0; col < 3; col++) ZK_TRY(zkmi_fr_batch_apply_key_dev(curve, d_ones, d_ident + (size_t)col * dom * W, dom, (const uint8_t*)firsts[col].v, (const uint8_t*)w.v));
        hipLaunchKernelGGL((k_psetup_sigma<FrC>), blocks(3 * dom), dim3(256), 0, st, d_ident, d_pred, d_cols + 5 * dom * W, (uint64_t)(3 * dom));
        ZK_HIP(hipGetLastError());
        ZK_HIP(hipStreamSynchronize(st));
        ms[1] = ms_since(t0);

        // ---- writeP4 for the eight columns and the Lagrange polynomials
        t0 = std::chrono::steady_clock::now();
        for (int c = 0; c < 8; c++) {
            uint32_t* sec = d_sec + (size_t)c * 5 * dom * W;
            ZK_TRY(zkmi_ntt_dev(curve, d_cols + (size_t)c * dom * W, sec, lg, 1, nullptr, nullptr));
            ZK_TRY(zkmi_ntt_padded_dev(curve, sec, dom, sec + dom * W, lg + 2, 0));
        }
        // d_ident is free again: its first column becomes the table w^(-e) / n
        ZK_TRY(zkmi_fr_batch_apply_key_dev(curve, d_ones, d_ident, dom, (const uint8_t*)n_inv.v, (const uint8_t*)w_inv.v));
        hipLaunchKernelGGL((k_psetup_lagrange<FrC>), blocks(n_poly * dom), dim3(256), 0, st, d_ident, d_lag, (uint32_t)n_poly, D);
        ZK_HIP(hipGetLastError());
        for (size_t i = 0; i < n_poly; i++) {
            uint32_t* rec = d_lag + i * 5 * dom * W;
            ZK_TRY(zkmi_ntt_padded_dev(curve, rec, dom, rec + dom * W, lg + 2, 0));
        }
        ZK_HIP(hipStreamSynchronize(st));
        ms[2] = ms_since(t0);
        return ZKMI_OK;
    }

    // the three shared downloads, enqueued on the stream: the caller adds its own and synchronises
    int download(uint8_t* const* q, uint8_t* sigma, uint8_t* lagrange) {
        hipStream_t st = ctx().stream;
        for (int c = 0; c < 5; c++) ZK_HIP(hipMemcpyAsync(q[c], d_sec + (size_t)c * 5 * dom * W, 5 * dom * 32, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipMemcpyAsync(sigma, d_sec + (size_t)5 * 5 * dom * W, 15 * dom * 32, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipMemcpyAsync(lagrange, d_lag, n_poly * 5 * dom * 32, hipMemcpyDeviceToHost, st));
        return ZKMI_OK;
    }
};

}  // namespace

}  // namespace zkmi
