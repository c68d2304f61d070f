// tools/fflonk_setup_hosttest.hip — the FFLONK gate lowering (csrc/fflonk_setup.hip: zkmi_fflonk_setup_lower_len, zkmi_fflonk_setup_lower) as a host
// program, for a run under the host sanitizers. It needs no device. Built with the translation unit itself, the rest of the library from libzkmi.so:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Isnarkjs_amd/csrc tools/fflonk_setup_hosttest.hip -o tools/bin/fflonk_setup_hosttest -Lsnarkjs_amd -lzkmi -Wl,-rpath,$PWD/snarkjs_amd
//   tools/bin/fflonk_setup_hosttest tests/golden/*.r1cs
// Per BN254 r1cs file: the lowering of the whole constraint section, of the same section in three pages cut at odd places (same result required), and of
// the section cut short by 1, 7 and 37 bytes and with nVars of 3 (each must be refused, none may read past its buffer). One line per file; exit 0 when all hold.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../snarkjs_amd/csrc/fflonk_setup.hip"

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
static Result run(const std::vector<std::vector<uint8_t>>& pages, uint32_t n_constraints, uint32_t n_vars, uint32_t n_public) {
    std::vector<const uint8_t*> ptr;
    std::vector<size_t> len;
    for (const auto& p : pages) { ptr.push_back(p.data()); len.push_back(p.size()); }
    zkmi_pages pg;
    pg.ptr = ptr.data(); pg.len = len.data(); pg.n_pages = (int)pages.size();
    Result r;
    r.rc = zkmi_fflonk_setup_lower_len(ZKMI_CURVE_BN128, pg, n_constraints, n_vars, n_public, r.cnt);
    if (r.rc) return r;
    r.additions.resize((size_t)r.cnt[1] * 72); r.selectors.resize((size_t)r.cnt[2] * 160); r.pred.resize((size_t)r.cnt[3] * 3);
    for (auto& m : r.maps) m.resize(r.cnt[2]);
    zkmi_plonk_lowered low = {r.cnt[0], r.cnt[1], r.cnt[2], r.cnt[3], r.additions.data(), r.maps[0].data(), r.maps[1].data(), r.maps[2].data(), r.selectors.data(), r.pred.data()};
    r.rc = zkmi_fflonk_setup_lower(ZKMI_CURVE_BN128, pg, n_constraints, n_vars, n_public, &low);
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
        if (n8 != 32 || file[head + 4] != 0x01 || file[head + 35] != 0x30) { printf("%s: not a BN254 r1cs, skipped\n", argv[a]); continue; }
        memcpy(hv, &file[head + 4 + n8], 16); memcpy(&n_constraints, &file[head + 4 + n8 + 24], 4);
        const uint32_t n_vars = hv[0], n_public = hv[1] + hv[2];
        const uint8_t* c = &file[cons];
        auto piece = [&](size_t lo, size_t hi) { return std::vector<uint8_t>(c + lo, c + hi); };
        const Result whole = run({piece(0, cons_len)}, n_constraints, n_vars, n_public);
        const size_t c1 = cons_len > 5 ? 5 : cons_len / 3, c2 = cons_len > 1001 ? 1001 : cons_len * 2 / 3;
        const Result paged = run({piece(0, c1), piece(c1, c2), piece(c2, cons_len)}, n_constraints, n_vars, n_public);
        int ok = whole.rc == ZKMI_OK && paged == whole;
        for (size_t cut : {(size_t)1, (size_t)7, (size_t)37})
            if (cons_len >= cut && n_constraints) ok &= run({piece(0, cons_len - cut)}, n_constraints, n_vars, n_public).rc == ZKMI_ERR_INVALID;
        if (n_vars > 3 && n_public < 3) ok &= run({piece(0, cons_len)}, n_constraints, 3, n_public).rc == ZKMI_ERR_INVALID;
        printf("%s: %s rows %u additions %u domain %u nVars %u\n", argv[a], ok ? "ok" : "FAILED", whole.cnt[2], whole.cnt[1], whole.cnt[3], whole.cnt[0]);
        bad += !ok;
    }
    return bad ? 1 : 0;
}
