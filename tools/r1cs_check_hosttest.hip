// tools/r1cs_check_hosttest.hip — the host passes of the witness check (csrc/r1cs_host.hpp: the offset pass over r1cs section 2, the batch cut) and the lane
// routines of its kernels (csrc/r1cs_check.cuh: r1cs_reduce256, r1cs_coef, r1cs_holds) as a host program. It needs no device and no library.
//   hipcc --offload-arch=gfx950 --cuda-host-only -O1 -std=c++17 -Isnarkjs_amd/csrc tools/r1cs_check_hosttest.hip -o tools/bin/r1cs_check_hosttest
// (add -Xarch_host -fsanitize=address,undefined for a run under the host sanitizers: the program has its own main). On the host the Montgomery product inside
// the lane routines is the plain operand-scanning one of r1cs_check.cuh; the reduction, the two products by R^2 and the comparison around it are the device's code.
// One request per line on stdin, one answer per line on stdout (tests/test_wtns_check_host.py):
//   offsets <n_constraints> <page lengths, comma separated, or -> <section as hex, or ->   ->  OK <used> <lc_first ...> | SHORT | TOOMANY
//        the section is copied into pages of exactly those lengths, each an allocation of its own (a read past a page is a sanitizer error)
//   reduce|coef <bn254|bls12381> <32 bytes as hex, little-endian>                         ->  v mod r | (v mod r) R^2 mod r, as hex
//   holds <bn254|bls12381> <a> <b> <c>      (Montgomery forms, hex)                       ->  1 | 0
//   cut <per_witness> <n_witnesses> <budget> <limit>                                      ->  witnesses per pass
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sstream>
#include <string>
#include <vector>
#include "r1cs_check.cuh"
#include "r1cs_host.hpp"

using namespace zkmi;

static int hexval(char c) { return c >= '0' && c <= '9' ? c - '0' : (c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1); }
static bool unhex(const std::string& s, std::vector<uint8_t>& out) {
    if (s == "-") return true;
    if (s.size() % 2) return false;
    for (size_t i = 0; i < s.size(); i += 2) {
        const int a = hexval(s[i]), b = hexval(s[i + 1]);
        if (a < 0 || b < 0) return false;
        out.push_back((uint8_t)(a * 16 + b));
    }
    return true;
}
static std::string hex(const uint8_t* p, size_t n) {
    std::string out;
    char b[3];
    for (size_t i = 0; i < n; i++) { snprintf(b, sizeof b, "%02x", p[i]); out += b; }
    return out;
}
template <class C> static bool fp_of(const std::string& s, Fp<C>& v) {
    std::vector<uint8_t> b;
    if (!unhex(s, b) || b.size() != 32) return false;
    memcpy(v.l, b.data(), 32);
    return true;
}
template <class C> static std::string field_op(const std::string& op, std::istringstream& in) {
    Fp<C> a, b, c;
    std::string s;
    if (!(in >> s) || !fp_of<C>(s, a)) return "ERR argument";
    if (op == "reduce") { r1cs_reduce256<C>(a); return hex((const uint8_t*)a.l, 32); }
    if (op == "coef") { a = r1cs_coef<C>(a); return hex((const uint8_t*)a.l, 32); }
    if (!(in >> s) || !fp_of<C>(s, b) || !(in >> s) || !fp_of<C>(s, c)) return "ERR argument";
    return r1cs_holds<C>(a, b, c) ? "1" : "0";
}
static std::string offsets(std::istringstream& in) {
    uint32_t n = 0;
    std::string lens, body;
    if (!(in >> n >> lens >> body)) return "ERR request";
    std::vector<uint8_t> sec;
    if (!unhex(body, sec)) return "ERR argument";
    std::vector<size_t> len;
    if (lens != "-") { std::istringstream ls(lens); std::string t; while (std::getline(ls, t, ',')) len.push_back((size_t)strtoull(t.c_str(), nullptr, 10)); }
    size_t total = 0;
    for (size_t l : len) total += l;
    if (total != sec.size()) return "ERR page lengths";
    std::vector<uint8_t*> ptr;
    size_t at = 0;
    for (size_t l : len) { uint8_t* p = (uint8_t*)malloc(l ? l : 1); if (l) memcpy(p, sec.data() + at, l); ptr.push_back(p); at += l; }
    zkmi_pages pg;
    pg.ptr = ptr.data(); pg.len = len.data(); pg.n_pages = (int)len.size();
    std::vector<uint32_t> first;
    uint64_t used = 0;
    const int rc = r1cs_lc_offsets(pg, n, first, &used);
    for (uint8_t* p : ptr) free(p);
    if (rc == R1CS_OFFSETS_SHORT) return "SHORT";
    if (rc == R1CS_OFFSETS_TOO_MANY) return "TOOMANY";
    std::string out = "OK " + std::to_string(used);
    for (uint32_t v : first) out += " " + std::to_string(v);
    return out;
}

int main() {
    std::string line;
    char buf[1 << 16];
    while (fgets(buf, sizeof buf, stdin)) {
        line = buf;
        while (!line.empty() && line.back() != '\n' && fgets(buf, sizeof buf, stdin)) line += buf;
        while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
        std::istringstream in(line);
        std::string op, field, out;
        in >> op;
        if (op == "offsets") out = offsets(in);
        else if (op == "cut") {
            uint64_t per = 0, budget = 0;
            uint32_t n = 0, limit = 0;
            out = (in >> per >> n >> budget >> limit) ? std::to_string(r1cs_batch_cut(per, n, budget, limit)) : "ERR request";
        } else if (op == "reduce" || op == "coef" || op == "holds") {
            in >> field;
            out = field == "bn254" ? field_op<Bn254Fr>(op, in) : (field == "bls12381" ? field_op<Bls12381Fr>(op, in) : "ERR field");
        } else out = "ERR request";
        printf("%s\n", out.c_str());
        fflush(stdout);
    }
    return 0;
}
