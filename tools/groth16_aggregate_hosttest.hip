// tools/groth16_aggregate_hosttest.hip — runs the aggregated Groth16 check of csrc/groth16_aggregate.cuh ON THE CPU, driven over stdin/stdout by
// tests/test_groth16_aggregate_host.py, which checks every result against tests/groth16_aggregate_vectors.py. The same source is compiled as for
// the device: __device__ is defined away below and the MAC is the compiler-scheduled one (ZKMI_MUL_VARIANT 1), exactly as
// tools/aggregate_verify_hosttest.hip does. The lanes of a batch run one after the other and their records are folded in order (the device folds
// them by trees; the group laws make the results the same).
//
// build: hipcc --offload-arch=gfx950 --cuda-host-only -O0 -std=c++17 -Isnarkjs_amd/csrc tools/groth16_aggregate_hosttest.hip -o tools/bin/groth16_aggregate_hosttest
// protocol: one request per line "<op> <curve 0|1> ...", one reply line (or "ERR ...").
//   agg c n_ic n_sig alpha(3) beta(6) gamma(6) delta(6) IC(3 n_ic) seed(64 hex digits, the bytes in order) n { A(3) B(6) C(3) pubs(n_sig) } x n
//       -> ok pair_ok S_X.x S_X.y S_C.x S_C.y s final_exp(F)[12, the oracle's w-basis] code_0 .. code_(n-1)
//   pow c e f[12]                        -> f^e by f12_pow3 (e below 2^192), 12 coefficients
#define ZKMI_MUL_VARIANT 1
#include <hip/hip_runtime.h>
#undef __device__
#define __device__
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include <sstream>
#include <iostream>
#include "pairing_host.hpp"
#include "groth16_aggregate.cuh"

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
    Fp<C> std_fp() { Words w = parse_hex(tok.at(at++), N); Fp<C> r; for (int i = 0; i < N; i++) r.l[i] = w[i]; return r; }
    Fp12<C> f12_in() {
        Fp<C> e[12];
        for (int k = 0; k < 12; k++) e[k] = fp_to_mont(std_fp());
        Fp<C> s = fp_zero<C>();
        s.l[0] = PairingCfg<C>::XI_S;
        s = fp_to_mont(s);
        Fp2<C> c[6];
        for (int k = 0; k < 6; k++) c[k] = Fp2<C>{fp_add(e[k], fp_mul(s, e[k + 6])), e[k + 6]};
        return Fp12<C>{Fp6<C>{c[0], c[2], c[4]}, Fp6<C>{c[1], c[3], c[5]}};
    }
    std::string f12_out(const Fp12<C>& a) {
        Fp<C> o[12];
        f12_to_wbasis(a, o);
        std::string s;
        for (int k = 0; k < 12; k++) s += (k ? " " : "") + hex(o[k].l, N);
        return s;
    }
    std::string run(const std::string& op) {
        if (op == "pow") {
            const Words e = parse_hex(tok.at(at++), 6);
            const uint64_t e3[3] = {e[0] | (uint64_t)e[1] << 32, e[2] | (uint64_t)e[3] << 32, e[4] | (uint64_t)e[5] << 32};
            return f12_out(f12_pow3(f12_in(), e3));
        }
        if (op == "agg") {
            const uint32_t n_ic = (uint32_t)std::stoul(tok.at(at++)), n_sig = (uint32_t)std::stoul(tok.at(at++));
            Words al, be, ga, de, ic;
            words(al, 3, N); words(be, 6, N); words(ga, 6, N); words(de, 6, N); words(ic, 3 * n_ic, N);
            constexpr int NL = miller_lines<C>();
            std::vector<Line<C>> tb(NL), tg(NL), td(NL);
            std::vector<Fp<C>> icm(2 * n_ic + 2);
            Fp12<C> mab;
            const uint32_t flags = vk_prepare(al.data(), be.data(), ga.data(), de.data(), ic.data(), n_ic, &K, icm.data(), tb.data(), tg.data(), td.data(), &mab);
            const VkView<C> vk{icm.data(), n_ic, tg.data(), td.data(), flags & 1u, (flags >> 1) & 1u, &mab};
            const std::string h = tok.at(at++);
            if (h.size() != 64) throw std::runtime_error("seed: 64 hex digits");
            uint8_t b[32];
            for (int i = 0; i < 32; i++) b[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
            uint64_t seed[4];
            memcpy(seed, b, 32);
            const size_t n = std::stoul(tok.at(at++));
            G16Part<C> S;
            g16_part_identity(S);
            std::string codes;
            bool all = true;
            for (size_t i = 0; i < n; i++) {
                Words rec, pubs;
                words(rec, 12, N); words(pubs, n_sig, 8);
                pubs.resize(pubs.size() + 8);
                G16Part<C> mine;
                const int code = g16_agg_lane_one(rec.data(), pubs.data(), n_sig, vk, &K, seed, (uint64_t)i, mine);
                // the block's three trees, one element at a time
                Fp12<C> f;
                g16_block_prod<C, 1>(&f, 0, f12_mul(S.f, mine.f));
                S.f = f;
                S.s.p = pt_add(S.s.p, mine.s.p);
                S.s.q = pt_add(S.s.q, mine.s.q);
                g16_add3(S.r, mine.r);
                all = all && code == AGG_ENTERED;
                codes += " " + std::to_string(code);
            }
            G16AggResult<C> res;
            memset(&res, 0, sizeof res);
            res.pair_ok = 1;
            res.gt[0] = 1;
            if (n) g16_agg_tail(S, vk, &K, true, &res);
            const uint32_t s6[6] = {(uint32_t)res.s[0], (uint32_t)(res.s[0] >> 32), (uint32_t)res.s[1], (uint32_t)(res.s[1] >> 32), (uint32_t)res.s[2], (uint32_t)(res.s[2] >> 32)};
            std::string out = std::to_string((all && res.pair_ok) ? 1 : 0) + " " + std::to_string(res.pair_ok) + " " + hex(res.sx, N) + " " + hex(res.sx + N, N) + " " +
                              hex(res.sc, N) + " " + hex(res.sc + N, N) + " " + hex(s6, 6);
            for (int k = 0; k < 12; k++) out += " " + hex(res.gt + k * N, N);
            return out + codes;
        }
        throw std::runtime_error("unknown op " + op);
    }
};

int main() {
    Run<Bn254Fq> bn;
    Run<Bls12381Fq> bls;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::vector<std::string> tok;
        std::string t;
        while (is >> t) tok.push_back(t);
        if (tok.size() < 2) { printf("ERR empty\n"); fflush(stdout); continue; }
        try {
            std::string op = tok[0];
            int curve = std::stoi(tok[1]);
            std::vector<std::string> rest(tok.begin() + 2, tok.end());
            std::string out;
            if (curve == 0) { bn.tok = rest; bn.at = 0; out = bn.run(op); }
            else { bls.tok = rest; bls.at = 0; out = bls.run(op); }
            printf("%s\n", out.c_str());
        } catch (const std::exception& e) {
            printf("ERR %s\n", e.what());
        }
        fflush(stdout);
    }
    return 0;
}
