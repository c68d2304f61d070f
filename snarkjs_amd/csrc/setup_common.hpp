// snarkjs_amd/csrc/setup_common.hpp — what the setups (groth16_setup.hip, plonk_setup.hip, fflonk_setup.hip) share on the host: the device memory of
// one call, a sequential reader over a paged buffer (the r1cs constraint section), the byte total of a paged buffer and, for the two gate lowerings,
// one linear combination of a constraint as the reference's reader leaves it. The lowering itself and the device steps that plonk_setup.hip and
// fflonk_setup.hip share are in gate_setup.hpp, which builds on this file.
#pragma once
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "host_field.hpp"
#include "zkmi_common.hpp"

namespace zkmi {

namespace {                                       // internal to each of the two units, as they were in groth16_setup.hip

struct DevMem {                                   // device memory of one call: freed on every return path
    const char* const who;                        // the entry point's name, the prefix of its error text
    std::vector<void*> blocks;
    explicit DevMem(const char* w) : who(w) {}
    ~DevMem() { for (void* p : blocks) (void)hipFree(p); }
    int get(size_t bytes, void** out) {
        *out = nullptr;
        hipError_t e = hipMalloc(out, bytes ? bytes : 16);
        if (e != hipSuccess) return fail(ZKMI_ERR_HIP, std::string(who) + ": hipMalloc: " + hipGetErrorString(e));
        blocks.push_back(*out);
        return ZKMI_OK;
    }
};

// sequential reader over a paged buffer
struct PageReader {
    const zkmi_pages& pg;
    int page = 0;
    size_t off = 0;
    explicit PageReader(const zkmi_pages& p) : pg(p) {}
    bool read(void* dst, size_t n) {
        uint8_t* d = (uint8_t*)dst;
        while (n) {
            while (page < pg.n_pages && off == pg.len[page]) { page++; off = 0; }
            if (page >= pg.n_pages) return false;
            const size_t k = std::min(n, pg.len[page] - off);
            if (d) { memcpy(d, pg.ptr[page] + off, k); d += k; }
            off += k; n -= k;
        }
        return true;
    }
    bool u32(uint32_t& v) { return read(&v, 4); }
    bool skip(size_t n) { return read(nullptr, n); }
};
inline size_t pages_bytes(const zkmi_pages& p) {
    size_t t = 0;
    for (int i = 0; i < p.n_pages; i++) t += p.len[i];
    return t;
}


// ---- the gate lowerings of plonk.setup and fflonk.setup
struct Term { uint32_t s; host::HFp<4> c; };
typedef std::vector<Term> Lc;                     // a linear combination as the reference holds it: keys ascending, one coefficient per key

// src/misc.js log2 on a 32-bit value
inline int ref_log2(uint32_t v) { return v ? 31 - __builtin_clz(v) : 0; }

// One linear combination of the r1cs constraint section (u32 n, then n x (u32 signal, 32-byte little-endian coefficient)) into `lc`, Montgomery
// coefficients; `raw` is scratch. `who` prefixes the error text.
inline int read_lc(PageReader& rd, const host::HField<4>& F, uint32_t n_vars, std::vector<Term>& raw, Lc& lc, const char* who) {
    typedef host::HField<4> HF;
    uint32_t n;
    if (!rd.u32(n)) return fail(ZKMI_ERR_INVALID, std::string(who) + ": the r1cs constraint section ends inside a constraint");
    raw.clear();
    bool sorted = true;
    for (uint32_t i = 0; i < n; i++) {
        Term t;
        if (!rd.u32(t.s) || !rd.read(t.c.v, 32)) return fail(ZKMI_ERR_INVALID, std::string(who) + ": the r1cs constraint section ends inside a constraint");
        if (t.s >= n_vars) return fail(ZKMI_ERR_INVALID, std::string(who) + ": a constraint names a signal beyond nVars");
        // a coefficient of r or more: the reference's reader (r1csfile readConstraints: F.fromRprLE) hands the raw 32 bytes to the WASM
        // toMontgomery, a Montgomery product with R^2 that ends in one conditional subtraction, so it keeps (c mod r) in Montgomery form for
        // every c < 2^256. Reducing first (at most 5 subtractions on BN254, 2 on BLS12-381) gives the same element.
        while (HF::cmp(t.c.v, F.p) >= 0) { uint64_t bw = 0; for (int j = 0; j < 4; j++) { host::u128 d = (host::u128)t.c.v[j] - F.p[j] - bw; t.c.v[j] = (uint64_t)d; bw = (uint64_t)(d >> 64) & 1; } }
        t.c = F.to_mont(t.c);
        if (!raw.empty() && raw.back().s >= t.s) sorted = false;
        raw.push_back(t);
    }
    // the reader keeps one coefficient per signal, the last one; `for (s in lc)` then walks the keys in ascending order
    if (!sorted) std::stable_sort(raw.begin(), raw.end(), [](const Term& x, const Term& y) { return x.s < y.s; });
    lc.clear();
    for (size_t i = 0; i < raw.size(); i++) if (i + 1 == raw.size() || raw[i + 1].s != raw[i].s) lc.push_back(raw[i]);
    return ZKMI_OK;
}

}  // namespace

}  // namespace zkmi
