// snarkjs_amd/csrc/groth16_setup.hip — host driver + C-ABI of the Groth16 setup (zkey new, src/zkey_new.js) on the device.
//
// Host side, one pass over the r1cs constraint section (variable-length records, src/zkey_new.js:203-288): every coefficient is reduced mod r,
// written to section 4 as value * R^2 mod r (:303-334) and recoded as sign and magnitude; the entries of the three matrices are then grouped
// by signal (counting sort) into the four column sets A, B1, B2 and IC|C, cut into segments and uploaded (groth16_setup.cuh runs them).
#include <string.h>
#include <algorithm>
#include <unordered_map>
#include "gconv.cuh"
#include "groth16_setup.cuh"
#include "host_field.hpp"
#include "setup_common.hpp"
#include "zkmi_common.hpp"

namespace zkmi {

namespace {

struct Mag { uint64_t v[4]; bool operator==(const Mag& o) const { return memcmp(v, o.v, sizeof v) == 0; } };
struct MagHash { size_t operator()(const Mag& m) const { uint64_t h = 0x9e3779b97f4a7c15ull; for (uint64_t x : m.v) h = (h ^ x) * 0xff51afd7ed558ccdull + (h >> 29); return (size_t)h; } };

constexpr uint32_t COEF_ZERO = 0xffffffffu;       // the term contributes nothing (its record in section 4 stays)

// entries of one constraint matrix in file order: signal, constraint, coefficient reference (bit 31: negated; low bits: 0 = magnitude 1, k = mags[k - 1])
struct Matrix { std::vector<uint32_t> sig, row, coef; };

struct Parsed {
    Matrix m[3];
    std::vector<Mag> mags;
    std::vector<uint16_t> mag_top;                // top bit of mags[k]
};

int top_bit(const Mag& m) {
    for (int i = 3; i >= 0; i--) if (m.v[i]) return 64 * i + 63 - __builtin_clzll(m.v[i]);
    return 0;
}

template <class FrC> int parse_constraints(const zkmi_groth16_setup_in& in, Parsed& P, uint8_t* sec4, size_t sec4_len) {
    typedef host::HField<4> HF;
    const HF F = HF::from_cfg<FrC>();
    const host::HFp<4> R3 = F.mul(F.R2(), F.R2());                     // mul(v, R^3) = v R^2
    const host::HFp<4> oneR2 = F.R2(), minusR2 = F.neg(F.R2());
    uint64_t half[4];                                                    // (r - 1) / 2
    for (int i = 0; i < 4; i++) half[i] = (F.p[i] >> 1) | (i < 3 ? F.p[i + 1] << 63 : 0);
    std::unordered_map<Mag, uint32_t, MagHash> seen;
    PageReader rd(in.constraints);
    uint8_t* w = sec4 + 4;
    uint8_t* const w_end = sec4 + sec4_len;
    uint64_t n_coef = 0;
    for (uint32_t c = 0; c < in.n_constraints; c++) {
        for (int k = 0; k < 3; k++) {
            uint32_t n;
            if (!rd.u32(n)) return fail(ZKMI_ERR_INVALID, "groth16_setup: the r1cs constraint section ends inside a constraint");
            Matrix& M = P.m[k];
            for (uint32_t i = 0; i < n; i++) {
                uint32_t s;
                host::HFp<4> v;
                if (!rd.u32(s) || !rd.read(v.v, 32)) return fail(ZKMI_ERR_INVALID, "groth16_setup: the r1cs constraint section ends inside a constraint");
                if (s >= in.n_vars) return fail(ZKMI_ERR_INVALID, "groth16_setup: a constraint names a signal beyond nVars");
                while (HF::cmp(v.v, F.p) >= 0) { uint64_t bw = 0; for (int j = 0; j < 4; j++) { host::u128 d = (host::u128)v.v[j] - F.p[j] - bw; v.v[j] = (uint64_t)d; bw = (uint64_t)(d >> 64) & 1; } }
                const bool neg = HF::cmp(v.v, half) > 0;
                Mag mg;
                if (neg) { const host::HFp<4> t = F.sub(F.zero(), v); memcpy(mg.v, t.v, 32); } else memcpy(mg.v, v.v, 32);
                const bool unit = mg.v[0] == 1 && !(mg.v[1] | mg.v[2] | mg.v[3]);
                uint32_t ref;
                if (unit) ref = neg ? 0x80000000u : 0u;
                else if (!(mg.v[0] | mg.v[1] | mg.v[2] | mg.v[3])) ref = COEF_ZERO;
                else {
                    auto it = seen.find(mg);
                    uint32_t id;
                    if (it != seen.end()) id = it->second;
                    else {
                        if (P.mags.size() >= 0x7ffffff0u) return fail(ZKMI_ERR_UNSUPPORTED, "groth16_setup: too many distinct coefficients");
                        P.mags.push_back(mg); P.mag_top.push_back((uint16_t)top_bit(mg));
                        id = (uint32_t)P.mags.size();
                        seen.emplace(mg, id);
                    }
                    ref = id | (neg ? 0x80000000u : 0u);
                }
                M.sig.push_back(s); M.row.push_back(c); M.coef.push_back(ref);
                if (k < 2) {                                             // section 4: A entries, then B entries, of every constraint
                    if (w + 44 > w_end) return fail(ZKMI_ERR_INVALID, "groth16_setup: coefficient buffer too small (zkmi_groth16_setup_coeffs_len)");
                    const uint32_t h[3] = {(uint32_t)k, c, s};
                    memcpy(w, h, 12);
                    const host::HFp<4> o = unit ? (neg ? minusR2 : oneR2) : F.mul(v, R3);
                    memcpy(w + 12, o.v, 32);
                    w += 44; n_coef++;
                }
            }
        }
    }
    for (uint32_t s = 0; s <= in.n_public; s++) {                        // the binding rows (:290-300)
        if (w + 44 > w_end) return fail(ZKMI_ERR_INVALID, "groth16_setup: coefficient buffer too small (zkmi_groth16_setup_coeffs_len)");
        const uint32_t h[3] = {0u, in.n_constraints + s, s};
        memcpy(w, h, 12); memcpy(w + 12, oneR2.v, 32);
        w += 44; n_coef++;
    }
    if (w != w_end || n_coef > 0xffffffffull) return fail(ZKMI_ERR_INVALID, "groth16_setup: coefficient buffer length does not match the constraints");
    const uint32_t nc = (uint32_t)n_coef;
    memcpy(sec4, &nc, 4);
    return ZKMI_OK;
}

// one source of terms of a column set: the entries of a matrix against the table that starts at base index `base0`
struct Stream { const Matrix* M; uint32_t base0; };

struct ColumnSet {
    std::vector<uint2> terms;
    std::vector<uint4> segs;                      // sorted for the launch
    std::vector<uint32_t> off;                    // column -> first partial sum (n_cols + 1)
};

// `bind0`: base index of the binding row of signal 0 (rows nConstraints + s, s <= nPublic), or ~0u for none
int build_columns(const Parsed& P, const std::vector<Stream>& streams, uint32_t n_cols, uint32_t n_public, uint32_t bind0, ColumnSet& out) {
    std::vector<uint64_t> start(n_cols + 1, 0);
    for (const Stream& st : streams)
        for (size_t k = 0; k < st.M->sig.size(); k++) if (st.M->coef[k] != COEF_ZERO) start[st.M->sig[k] + 1]++;
    if (bind0 != ~0u) for (uint32_t s = 0; s <= n_public; s++) start[s + 1]++;
    for (uint32_t s = 0; s < n_cols; s++) start[s + 1] += start[s];
    const uint64_t n_terms = start[n_cols];
    if (n_terms >= 0xffffffffull) return fail(ZKMI_ERR_UNSUPPORTED, "groth16_setup: more than 2^32 terms in one section");
    out.terms.resize(n_terms);
    std::vector<uint16_t> top(n_terms);
    std::vector<uint64_t> fill(start.begin(), start.end() - 1);
    for (const Stream& st : streams)
        for (size_t k = 0; k < st.M->sig.size(); k++) {
            const uint32_t ref = st.M->coef[k];
            if (ref == COEF_ZERO) continue;
            const uint64_t at = fill[st.M->sig[k]]++;
            out.terms[at] = make_uint2((st.base0 + st.M->row[k]) | (ref & 0x80000000u), ref & 0x7fffffffu);
            top[at] = (ref & 0x7fffffffu) ? P.mag_top[(ref & 0x7fffffffu) - 1] : 0;
        }
    if (bind0 != ~0u) for (uint32_t s = 0; s <= n_public; s++) { const uint64_t at = fill[s]++; out.terms[at] = make_uint2(bind0 + s, 0u); top[at] = 0; }
    out.off.assign(n_cols + 1, 0);
    std::vector<uint32_t> idx;
    std::vector<uint2> tmp_t;
    std::vector<uint16_t> tmp_b;
    for (uint32_t s = 0; s < n_cols; s++) {
        const uint64_t b = start[s], e = start[s + 1];
        out.off[s] = (uint32_t)out.segs.size();
        if (e - b > (uint64_t)SETUP_SEG) {                               // a cut column: widest coefficients first, so that they share segments
            bool wide = false;
            for (uint64_t k = b; k < e && !wide; k++) wide = top[k] != 0;
            if (wide) {
                idx.resize(e - b);
                for (size_t k = 0; k < idx.size(); k++) idx[k] = (uint32_t)k;
                std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return top[b + x] > top[b + y]; });
                tmp_t.assign(out.terms.begin() + b, out.terms.begin() + e);
                tmp_b.assign(top.begin() + b, top.begin() + e);
                for (size_t k = 0; k < idx.size(); k++) { out.terms[b + k] = tmp_t[idx[k]]; top[b + k] = tmp_b[idx[k]]; }
            }
        }
        for (uint64_t k = b; k < e; k += SETUP_SEG) {
            const uint32_t n = (uint32_t)std::min<uint64_t>(SETUP_SEG, e - k);
            uint16_t t = 0;
            for (uint32_t j = 0; j < n; j++) t = std::max(t, top[k + j]);
            out.segs.push_back(make_uint4((uint32_t)k, n, t, (uint32_t)out.segs.size()));
        }
    }
    out.off[n_cols] = (uint32_t)out.segs.size();
    std::sort(out.segs.begin(), out.segs.end(), [](const uint4& a, const uint4& b) { return a.z != b.z ? a.z > b.z : (a.y != b.y ? a.y > b.y : a.w < b.w); });
    return ZKMI_OK;
}

double g_setup_ms[5] = {0, 0, 0, 0, 0};           // A, B1, B2, IC|C, H differences: device time of the last call

// evaluate, fold and normalise one column set; d_out: n_cols affine points
template <class F> int run_columns(const ColumnSet& cs, uint32_t n_cols, const uint32_t* d_bases, const uint32_t* d_mags, uint32_t* d_out, double* ms) {
    constexpr int FW = FieldWords<F>::value;
    Ctx& cx = ctx();
    hipStream_t st = cx.stream;
    DevMem dm("groth16_setup");
    const uint32_t n_seg = (uint32_t)cs.segs.size();
    void *d_terms, *d_segs, *d_off, *d_part;
    ZK_TRY(dm.get(cs.terms.size() * sizeof(uint2), &d_terms));
    ZK_TRY(dm.get((size_t)n_seg * sizeof(uint4), &d_segs));
    ZK_TRY(dm.get((size_t)n_seg * 4 * FW * 4, &d_part));
    if (!cs.terms.empty()) ZK_HIP(hipMemcpyAsync(d_terms, cs.terms.data(), cs.terms.size() * sizeof(uint2), hipMemcpyHostToDevice, st));
    if (n_seg) ZK_HIP(hipMemcpyAsync(d_segs, cs.segs.data(), (size_t)n_seg * sizeof(uint4), hipMemcpyHostToDevice, st));
    // fold levels: runs of at most SETUP_FOLD partial sums until every column holds one
    std::vector<std::vector<uint32_t>> levels;
    std::vector<uint32_t> cnt(n_cols);
    for (uint32_t s = 0; s < n_cols; s++) cnt[s] = cs.off[s + 1] - cs.off[s];
    for (;;) {
        const uint32_t mx = n_cols ? *std::max_element(cnt.begin(), cnt.end()) : 0;
        std::vector<uint32_t> off;
        uint32_t pos = 0;
        off.push_back(0);
        if (mx <= (uint32_t)SETUP_FOLD) {
            for (uint32_t s = 0; s < n_cols; s++) { pos += cnt[s]; off.push_back(pos); }
            levels.push_back(std::move(off));
            break;
        }
        for (uint32_t s = 0; s < n_cols; s++) {
            uint32_t left = cnt[s], g = 0;
            while (left) { const uint32_t k = std::min<uint32_t>(left, SETUP_FOLD); pos += k; off.push_back(pos); left -= k; g++; }
            cnt[s] = g;
        }
        levels.push_back(std::move(off));
    }
    std::vector<void*> d_lv(levels.size());
    for (size_t l = 0; l < levels.size(); l++) {
        ZK_TRY(dm.get(levels[l].size() * 4, &d_lv[l]));
        ZK_HIP(hipMemcpyAsync(d_lv[l], levels[l].data(), levels[l].size() * 4, hipMemcpyHostToDevice, st));
    }
    void* d_xyzz[2] = {nullptr, nullptr};
    const size_t widest = levels.size() > 1 ? std::max<size_t>(levels[0].size() - 1, n_cols) : n_cols;
    ZK_TRY(dm.get(widest * 4 * FW * 4, &d_xyzz[0]));
    if (levels.size() > 1) ZK_TRY(dm.get(widest * 4 * FW * 4, &d_xyzz[1]));
    ZK_HIP(hipStreamSynchronize(st));                                    // the level tables are locals
    hipEvent_t e0, e1;
    ZK_HIP(hipEventCreate(&e0));
    ZK_HIP(hipEventCreate(&e1));
    ZK_HIP(hipEventRecord(e0, st));
    if (n_seg) hipLaunchKernelGGL((k_setup_eval<F, SETUP_T>), dim3((n_seg + SETUP_T - 1) / SETUP_T), dim3(SETUP_T), 0, st, d_bases, (const uint2*)d_terms, (const uint4*)d_segs, d_mags,
                                  (uint32_t*)d_part, n_seg);
    const uint32_t* src = (const uint32_t*)d_part;
    int flip = 0;
    for (size_t l = 0; l < levels.size(); l++) {
        const uint32_t n_out = (uint32_t)levels[l].size() - 1;
        if (n_out) hipLaunchKernelGGL((k_setup_fold<F, SETUP_T>), dim3((n_out + SETUP_T - 1) / SETUP_T), dim3(SETUP_T), 0, st, src, (const uint32_t*)d_lv[l], (uint32_t*)d_xyzz[flip], n_out);
        src = (const uint32_t*)d_xyzz[flip];
        flip ^= 1;
    }
    if (n_cols) {
        const uint32_t lanes = (n_cols + SETUP_INV - 1) / SETUP_INV;
        hipLaunchKernelGGL((k_setup_affine<F>), dim3((lanes + 255) / 256), dim3(256), 0, st, src, d_out, n_cols);
    }
    ZK_HIP(hipEventRecord(e1, st));
    hipError_t err = hipStreamSynchronize(st);
    float t = 0;
    if (err == hipSuccess) err = hipEventElapsedTime(&t, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    ZK_HIP(err);
    ZK_HIP(hipGetLastError());
    *ms = t;
    return ZKMI_OK;
}

template <class FqC, class FrC> int setup_run(const zkmi_groth16_setup_in& in, const zkmi_groth16_setup_out& out) {
    typedef Fp<FqC> F1;
    typedef Fp2<FqC> F2;
    constexpr size_t sG1 = 2 * FqC::N * 4, sG2 = 2 * sG1;
    Ctx& cx = ctx();
    hipStream_t st = cx.stream;
    const size_t dom = in.domain_size, nv = in.n_vars, npub = in.n_public;
    if (out.ic_len != (npub + 1) * sG1 || out.a_len != nv * sG1 || out.b1_len != nv * sG1 || out.b2_len != nv * sG2 || out.c_len != (nv - npub - 1) * sG1 ||
        out.h_len != (size_t)in.n_h * sG1)
        return fail(ZKMI_ERR_INVALID, "groth16_setup: an output buffer does not have the length of its section");
    if (!out.ic || !out.coeffs || !out.a || !out.b1 || !out.b2 || (out.c_len && !out.c) || !out.h) return fail(ZKMI_ERR_INVALID, "groth16_setup: null output buffer");
    if (pages_bytes(in.tau_g1) != dom * sG1 || pages_bytes(in.alpha_tau_g1) != dom * sG1 || pages_bytes(in.beta_tau_g1) != dom * sG1 || pages_bytes(in.tau_g2) != dom * sG2)
        return fail(ZKMI_ERR_INVALID, "groth16_setup: a Lagrange slice does not hold domainSize points");
    if (pages_bytes(in.tau_g1_powers) != (dom + in.n_h) * sG1) return fail(ZKMI_ERR_INVALID, "groth16_setup: the tauG1 slice must hold domainSize + n_h points");

    Parsed P;
    ZK_TRY(parse_constraints<FrC>(in, P, out.coeffs, out.coeffs_len));

    DevMem dm("groth16_setup");
    uint32_t *d_g1, *d_g2, *d_mags, *d_pts;
    ZK_TRY(dm.get(3 * dom * sG1, (void**)&d_g1));                       // tauG1 | alphaTauG1 | betaTauG1
    ZK_TRY(dm.get(dom * sG2, (void**)&d_g2));
    ZK_TRY(dm.get(P.mags.size() * 32, (void**)&d_mags));
    ZK_TRY(dm.get(nv * sG2, (void**)&d_pts));
    ZK_TRY(upload_pages(in.tau_g1, dom * sG1, d_g1));
    ZK_TRY(upload_pages(in.alpha_tau_g1, dom * sG1, (uint8_t*)d_g1 + dom * sG1));
    ZK_TRY(upload_pages(in.beta_tau_g1, dom * sG1, (uint8_t*)d_g1 + 2 * dom * sG1));
    ZK_TRY(upload_pages(in.tau_g2, dom * sG2, d_g2));
    if (!P.mags.empty()) ZK_HIP(hipMemcpyAsync(d_mags, P.mags.data(), P.mags.size() * 32, hipMemcpyHostToDevice, st));
    ZK_HIP(hipStreamSynchronize(st));

    const uint32_t D = in.domain_size, NC = in.n_constraints;
    {   // A: the A column over tauG1 plus the binding rows
        ColumnSet cs;
        ZK_TRY(build_columns(P, {{&P.m[0], 0u}}, in.n_vars, in.n_public, NC, cs));
        ZK_TRY(run_columns<F1>(cs, in.n_vars, d_g1, d_mags, d_pts, &g_setup_ms[0]));
        ZK_HIP(hipMemcpy(out.a, d_pts, out.a_len, hipMemcpyDeviceToHost));
    }
    {   // B1 and B2: the B column over tauG1 / tauG2 (one column set, two groups)
        ColumnSet cs;
        ZK_TRY(build_columns(P, {{&P.m[1], 0u}}, in.n_vars, in.n_public, ~0u, cs));
        ZK_TRY(run_columns<F1>(cs, in.n_vars, d_g1, d_mags, d_pts, &g_setup_ms[1]));
        ZK_HIP(hipMemcpy(out.b1, d_pts, out.b1_len, hipMemcpyDeviceToHost));
        ZK_TRY(run_columns<F2>(cs, in.n_vars, d_g2, d_mags, d_pts, &g_setup_ms[2]));
        ZK_HIP(hipMemcpy(out.b2, d_pts, out.b2_len, hipMemcpyDeviceToHost));
    }
    {   // IC | C: A over betaTauG1, B over alphaTauG1, C over tauG1, the binding rows over betaTauG1
        ColumnSet cs;
        ZK_TRY(build_columns(P, {{&P.m[0], 2 * D}, {&P.m[1], D}, {&P.m[2], 0u}}, in.n_vars, in.n_public, 2 * D + NC, cs));
        ZK_TRY(run_columns<F1>(cs, in.n_vars, d_g1, d_mags, d_pts, &g_setup_ms[3]));
        ZK_HIP(hipMemcpy(out.ic, d_pts, out.ic_len, hipMemcpyDeviceToHost));
        if (out.c_len) ZK_HIP(hipMemcpy(out.c, (uint8_t*)d_pts + out.ic_len, out.c_len, hipMemcpyDeviceToHost));
    }
    {   // the H points of the circuit hash: tauG1[i + domain] - tauG1[i], affine, LEM -> U
        const uint32_t n = in.n_h;
        uint32_t *d_tau, *d_x, *d_aff, *d_u;
        ZK_TRY(dm.get((dom + n) * sG1, (void**)&d_tau));
        ZK_TRY(dm.get((size_t)n * 2 * sG1, (void**)&d_x));
        ZK_TRY(dm.get((size_t)n * sG1, (void**)&d_aff));
        ZK_TRY(dm.get((size_t)n * sG1, (void**)&d_u));
        ZK_TRY(upload_pages(in.tau_g1_powers, (dom + n) * sG1, d_tau));
        hipEvent_t e0, e1;
        ZK_HIP(hipEventCreate(&e0));
        ZK_HIP(hipEventCreate(&e1));
        ZK_HIP(hipEventRecord(e0, st));
        if (n) {
            hipLaunchKernelGGL((k_setup_hdiff<F1>), dim3((n + 255) / 256), dim3(256), 0, st, d_tau, d_x, n, D);
            const uint32_t lanes = (n + SETUP_INV - 1) / SETUP_INV;
            hipLaunchKernelGGL((k_setup_affine<F1>), dim3((lanes + 255) / 256), dim3(256), 0, st, d_x, d_aff, n);
            const uint64_t ne = (uint64_t)n * 2;
            hipLaunchKernelGGL((k_gconv_elems<FqC>), dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, d_aff, d_u, ne, 1, 1);
        }
        ZK_HIP(hipEventRecord(e1, st));
        hipError_t err = hipMemcpyAsync(out.h, d_u, out.h_len, hipMemcpyDeviceToHost, st);
        if (err == hipSuccess) err = hipStreamSynchronize(st);
        float t = 0;
        if (err == hipSuccess) err = hipEventElapsedTime(&t, e0, e1);
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        ZK_HIP(err);
        ZK_HIP(hipGetLastError());
        g_setup_ms[4] = t;
    }
    return ZKMI_OK;
}

int setup_check(const zkmi_groth16_setup_in* in) {
    if (!in) return fail(ZKMI_ERR_INVALID, "groth16_setup: null descriptor");
    if (in->curve != ZKMI_CURVE_BN128 && in->curve != ZKMI_CURVE_BLS12381) return fail(ZKMI_ERR_INVALID, "groth16_setup: unknown curve");
    const uint64_t d = in->domain_size;
    if (d < 2 || (d & (d - 1)) || d > (1ull << 28)) return fail(ZKMI_ERR_INVALID, "groth16_setup: domainSize must be a power of two, at most 2^28");
    if ((uint64_t)in->n_constraints + in->n_public + 1 > d) return fail(ZKMI_ERR_INVALID, "groth16_setup: nConstraints + nPublic + 1 exceeds domainSize");
    if (in->n_vars <= in->n_public) return fail(ZKMI_ERR_INVALID, "groth16_setup: nVars must exceed nPublic");
    if (in->n_h != d - 1 && in->n_h != d) return fail(ZKMI_ERR_INVALID, "groth16_setup: n_h must be domainSize - 1 or domainSize");
    return ZKMI_OK;
}

}  // namespace

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zkmi_groth16_setup_coeffs_len(zkmi_pages constraints, uint32_t n_constraints, uint32_t n_public, size_t* len) {
    if (!len) return fail(ZKMI_ERR_INVALID, "groth16_setup_coeffs_len: null result");
    PageReader rd(constraints);
    uint64_t n_coef = (uint64_t)n_public + 1;
    for (uint32_t c = 0; c < n_constraints; c++)
        for (int k = 0; k < 3; k++) {
            uint32_t n;
            if (!rd.u32(n) || !rd.skip((size_t)n * 36)) return fail(ZKMI_ERR_INVALID, "groth16_setup: the r1cs constraint section ends inside a constraint");
            if (k < 2) n_coef += n;
        }
    *len = 4 + (size_t)n_coef * 44;
    return ZKMI_OK;
}

int zkmi_groth16_setup_coeffs(int curve, zkmi_pages constraints, uint32_t n_constraints, uint32_t n_vars, uint32_t n_public, uint8_t* out, size_t out_len) {
    if (curve != ZKMI_CURVE_BN128 && curve != ZKMI_CURVE_BLS12381) return fail(ZKMI_ERR_INVALID, "groth16_setup: unknown curve");
    if (!out || out_len < 4) return fail(ZKMI_ERR_INVALID, "groth16_setup: coefficient buffer too small (zkmi_groth16_setup_coeffs_len)");
    zkmi_groth16_setup_in in;
    memset(&in, 0, sizeof in);
    in.curve = curve; in.n_constraints = n_constraints; in.n_vars = n_vars; in.n_public = n_public; in.constraints = constraints;
    Parsed P;
    return curve == ZKMI_CURVE_BN128 ? parse_constraints<Bn254Fr>(in, P, out, out_len) : parse_constraints<Bls12381Fr>(in, P, out, out_len);
}

int zkmi_groth16_setup(const zkmi_groth16_setup_in* in, const zkmi_groth16_setup_out* out) {
    ZK_TRY(require_ctx());
    ZK_TRY(setup_check(in));
    if (!out) return fail(ZKMI_ERR_INVALID, "groth16_setup: null output descriptor");
    if (pipeline_busy()) return fail(ZKMI_ERR_INVALID, "groth16_setup: a pipeline slot holds work in flight (collect it first)");
    return in->curve == ZKMI_CURVE_BN128 ? setup_run<Bn254Fq, Bn254Fr>(*in, *out) : setup_run<Bls12381Fq, Bls12381Fr>(*in, *out);
}

int zkmi_groth16_setup_phase_ms(double* out5) {
    if (!out5) return fail(ZKMI_ERR_INVALID, "groth16_setup_phase_ms: null result");
    for (int i = 0; i < 5; i++) out5[i] = g_setup_ms[i];
    return ZKMI_OK;
}

}  // extern "C"
