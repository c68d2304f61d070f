// tools/gate_setup_hosttest.hip — the gate lowering that the PLONK and the FFLONK setup share (csrc/gate_setup.hpp: lower_len_body, lower_body, the
// bodies of zkmi_*_setup_lower_len and zkmi_*_setup_lower) as a host program, for a run under the host sanitizers. It needs no device. Built with the
// header itself, the rest of the library from libzkmi.so:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Isnarkjs_amd/csrc tools/gate_setup_hosttest.hip -o tools/bin/gate_setup_hosttest -Lsnarkjs_amd -lzkmi -Wl,-rpath,$PWD/snarkjs_amd
//   tools/bin/gate_setup_hosttest tests/golden/*.r1cs
// Per r1cs file and rule set (PLONK's on the file's own curve, FFLONK's on BN254 files): the lowering of the whole constraint section, which must be what
// the library's own entry point gives; of the same section in three pages cut at odd places (same result required); and of the section cut short by 1, 7
// and 37 bytes and with nVars of 3 (each must be refused, none may read past its buffer). One line per file and rule set; exit 0 when all hold.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../snarkjs_amd/csrc/gate_setup.hpp"

using namespace zkmi;

// the two rule sets as plonk_setup.hip and fflonk_setup.hip hold them; the comparison with the library's entry points keeps them in step
typedef int (*lower_len_fn)(int, zkmi_pages, uint32_t, uint32_t, uint32_t, uint32_t*);
typedef int (*lower_fn)(int, zkmi_pages, uint32_t, uint32_t, uint32_t, const zkmi_plonk_lowered*);
struct Protocol { GateRules rules; lower_len_fn lib_len; lower_fn lib_lower; };
static const Protocol PLONK = {{"plonk_setup", false, 0, {1, 2, 0, 3, 4}}, zkmi_plonk_setup_lower_len, zkmi_plonk_setup_lower};
static const Protocol FFLONK = {{"fflonk_setup", true, 2, {0, 1, 2, 3, 4}}, zkmi_fflonk_setup_lower_len, zkmi_fflonk_setup_lower};

struct Result {
    int rc;
    uint32_t cnt[4];
    std::vector<uint8_t> additions, selectors;
    std::vector<uint32_t> maps[3], pred;
    bool operator==(const Result& o) const {
        return rc == o.rc && !memcmp(cnt, o.cnt, sizeof cnt) && additions == o.additions && selectors == o.selectors && maps[0] == o.maps[0] && maps[1] == o.maps[1] &&
               maps[2] == o.maps[2] && pred == o.pred;
    }
};

// every page is its own heap block of exactly its length, so that a read past a page is a read past an allocation
// through_lib: the library's entry points instead of the header's bodies
static Result run(const Protocol& P, int curve, bool through_lib, const std::vector<std::vector<uint8_t>>& pages, uint32_t n_constraints, uint32_t n_vars, uint32_t n_public) {
    const HF F = curve == ZKMI_CURVE_BN128 ? HF::from_cfg<Bn254Fr>() : HF::from_cfg<Bls12381Fr>();
    double ms = 0;
    std::vector<const uint8_t*> ptr;
    std::vector<size_t> len;
    for (const auto& p : pages) { ptr.push_back(p.data()); len.push_back(p.size()); }
    zkmi_pages pg;
    pg.ptr = ptr.data(); pg.len = len.data(); pg.n_pages = (int)pages.size();
    Result r;
    r.rc = through_lib ? P.lib_len(curve, pg, n_constraints, n_vars, n_public, r.cnt) : lower_len_body(P.rules, F, pg, n_constraints, n_vars, n_public, r.cnt, ms);
    if (r.rc) return r;
    r.additions.resize((size_t)r.cnt[1] * 72); r.selectors.resize((size_t)r.cnt[2] * 160); r.pred.resize((size_t)r.cnt[3] * 3);
    for (auto& m : r.maps) m.resize(r.cnt[2]);
    zkmi_plonk_lowered low = {r.cnt[0], r.cnt[1], r.cnt[2], r.cnt[3], r.additions.data(), r.maps[0].data(), r.maps[1].data(), r.maps[2].data(), r.selectors.data(), r.pred.data()};
    r.rc = through_lib ? P.lib_lower(curve, pg, n_constraints, n_vars, n_public, &low) : lower_body(P.rules, F, pg, n_constraints, n_vars, n_public, &low, ms);
    return r;
}

int main(int argc, char** argv) {
    int bad = 0;
    for (int a = 1; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { printf("%s: cannot open\n", argv[a]); bad++; continue; }
        std::vector<uint8_t> file;
        uint8_t buf[65536];
        for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + k);
        fclose(f);
        if (file.size() < 12 || memcmp(file.data(), "r1cs", 4)) { printf("%s: not an r1cs file\n", argv[a]); bad++; continue; }
        uint32_t n_sections; memcpy(&n_sections, &file[8], 4);
        size_t off = 12, head = 0, cons = 0, cons_len = 0;
        for (uint32_t i = 0; i < n_sections && off + 12 <= file.size(); i++) {
            uint32_t typ; uint64_t ln; memcpy(&typ, &file[off], 4); memcpy(&ln, &file[off + 4], 8);
            if (typ == 1) head = off + 12;
            if (typ == 2) { cons = off + 12; cons_len = ln; }
            off += 12 + ln;
        }
        uint32_t n8, hv[4], n_constraints;
        memcpy(&n8, &file[head], 4);
        const bool bn254 = n8 == 32 && file[head + 4] == 0x01 && file[head + 35] == 0x30, bls = n8 == 32 && file[head + 4] == 0x01 && file[head + 35] == 0x73;
        if (!bn254 && !bls) { printf("%s: neither a BN254 nor a BLS12-381 r1cs\n", argv[a]); bad++; continue; }
        const int curve = bn254 ? ZKMI_CURVE_BN128 : ZKMI_CURVE_BLS12381;
        memcpy(hv, &file[head + 4 + n8], 16); memcpy(&n_constraints, &file[head + 4 + n8 + 24], 4);
        const uint32_t n_vars = hv[0], n_public = hv[1] + hv[2];
        const uint8_t* c = &file[cons];
        auto piece = [&](size_t lo, size_t hi) { return std::vector<uint8_t>(c + lo, c + hi); };
        for (const Protocol* P : {&PLONK, &FFLONK}) {
            if (P == &FFLONK && !bn254) continue;                          // fflonk.setup is BN254 only
            const Result whole = run(*P, curve, false, {piece(0, cons_len)}, n_constraints, n_vars, n_public);
            int ok = whole.rc == ZKMI_OK && run(*P, curve, true, {piece(0, cons_len)}, n_constraints, n_vars, n_public) == whole;
            const size_t c1 = cons_len > 5 ? 5 : cons_len / 3, c2 = cons_len > 1001 ? 1001 : cons_len * 2 / 3;
            ok &= run(*P, curve, false, {piece(0, c1), piece(c1, c2), piece(c2, cons_len)}, n_constraints, n_vars, n_public) == whole;
            for (size_t cut : {(size_t)1, (size_t)7, (size_t)37})
                if (cons_len >= cut && n_constraints) ok &= run(*P, curve, false, {piece(0, cons_len - cut)}, n_constraints, n_vars, n_public).rc == ZKMI_ERR_INVALID;
            if (n_vars > 3 && n_public < 3) ok &= run(*P, curve, false, {piece(0, cons_len)}, n_constraints, 3, n_public).rc == ZKMI_ERR_INVALID;
            printf("%s %s: %s rows %u additions %u domain %u nVars %u\n", argv[a], P->rules.who, ok ? "ok" : "FAILED", whole.cnt[2], whole.cnt[1], whole.cnt[3], whole.cnt[0]);
            bad += !ok;
        }
    }
    return bad ? 1 : 0;
}
