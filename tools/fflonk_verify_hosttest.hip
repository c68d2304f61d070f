// tools/fflonk_verify_hosttest.hip — runs the FFLONK verification code of csrc/fflonk_verify.cuh ON THE CPU, driven over stdin/stdout by
// tests/test_fflonk_verify_host.py, which checks every result against oracle/fflonk_verify_oracle.py and the pairing oracle. The same source
// is compiled as for the device: __device__ is defined away below and the MAC is the compiler-scheduled one (ZKMI_MUL_VARIANT 1), exactly as
// tools/plonk_verify_hosttest.hip does for plonk_verify.cuh.
//
// build: hipcc --offload-arch=gfx950 --cuda-host-only -O0 -std=c++17 -Isnarkjs_amd/csrc tools/fflonk_verify_hosttest.hip -o tools/bin/fflonk_verify_hosttest
// protocol: one request per line "<op> <curve 0> ...", one reply line (or "ERR ...").
//   verify c power n_public omega_mont k1 k2 w3 w4 w8 wr C0 (x y z) X_2 (x0 x1 y0 y1 z0 z1) C1 C2 W1 W2 (4 x (x y z)) evals (15) pubs (n_public)
//                                     -> code beta gamma xi alpha y r0 r1 r2 A1.x A1.y B1.x B1.y c0_bad   (hex integers; code and c0_bad decimal)
#define ZKMI_MUL_VARIANT 1
#include <hip/hip_runtime.h>
#undef __device__
#define __device__
#include <stdio.h>
#include <string>
#include <vector>
#include <sstream>
#include <iostream>
#include "pairing_host.hpp"
#include "fflonk_verify.cuh"

using namespace zkmi;

typedef std::vector<uint32_t> Words;

static Words parse_hex(const std::string& h, int nw) {
    Words w(nw, 0);
    int bit = 0;
    for (int i = (int)h.size() - 1; i >= 0; i--, bit += 4) {
        char ch = h[i];
        uint32_t d = (ch >= '0' && ch <= '9') ? ch - '0' : (ch >= 'a' && ch <= 'f') ? ch - 'a' + 10 : ch - 'A' + 10;
        if (d && bit / 32 >= nw) throw std::runtime_error("value too wide");
        if (bit / 32 < nw) w[bit / 32] |= d << (bit % 32);
    }
    return w;
}
static std::string hex(const uint32_t* w, int nw) {
    static const char* D = "0123456789abcdef";
    std::string s;
    for (int i = nw - 1; i >= 0; i--)
        for (int k = 28; k >= 0; k -= 4) s += D[(w[i] >> k) & 15];
    size_t z = s.find_first_not_of('0');
    return z == std::string::npos ? "0" : s.substr(z);
}

template <class C> struct Run {
    static constexpr int N = C::N;
    PairingConsts<C> K;
    std::vector<std::string> tok;
    size_t at = 0;
    Run() { pairing_consts_host(K); }
    void words(Words& out, int count, int nw) { for (int k = 0; k < count; k++) { Words w = parse_hex(tok.at(at++), nw); out.insert(out.end(), w.begin(), w.end()); } }
    std::string run(const std::string& op) {
        if (op == "verify") {
            const uint32_t power = (uint32_t)std::stoul(tok.at(at++)), n_public = (uint32_t)std::stoul(tok.at(at++));
            Words om, consts, c0, x2, rec, pubs;
            words(om, 1, 8); words(consts, 6, 8); words(c0, 3, N); words(x2, 6, N); words(rec, 12, N); words(rec, FFLONK_EVALS, 8); words(pubs, n_public, 8);
            pubs.resize(pubs.size() + 8);
            constexpr int NL = miller_lines<C>();
            std::vector<Line<C>> tx(NL), tg(NL);
            FflonkVk<C> vk;
            fflonk_vk_prepare(c0.data(), x2.data(), consts.data(), om.data(), power, n_public, &K, &vk, tx.data(), tg.data());
            if (vk.bad) throw std::runtime_error("X_2 not on the curve");
            FflonkVkView<C> V{&vk, tx.data(), tg.data()};
            FflonkTrace<C> tr;
            memset(&tr, 0, sizeof tr);
            const int code = fflonk_verify_one(rec.data(), pubs.data(), V, &K, &tr);
            std::string s = std::to_string(code);
            for (int j = 0; j < 8; j++) s += " " + hex(tr.fr[j], 8);
            return s + " " + hex(tr.a1, N) + " " + hex(tr.a1 + N, N) + " " + hex(tr.b1, N) + " " + hex(tr.b1 + N, N) + " " + std::to_string(vk.c0_bad);
        }
        throw std::runtime_error("unknown op " + op);
    }
};

int main() {
    Run<Bn254Fq> bn;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::vector<std::string> tok;
        std::string t;
        while (is >> t) tok.push_back(t);
        if (tok.size() < 2) { printf("ERR empty\n"); fflush(stdout); continue; }
        try {
            if (std::stoi(tok[1]) != 0) throw std::runtime_error("FFLONK verification serves BN254 only");
            bn.tok.assign(tok.begin() + 2, tok.end());
            bn.at = 0;
            printf("%s\n", bn.run(tok[0]).c_str());
        } catch (const std::exception& e) {
            printf("ERR %s\n", e.what());
        }
        fflush(stdout);
    }
    return 0;
}
