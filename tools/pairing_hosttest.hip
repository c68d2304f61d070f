// tools/pairing_hosttest.hip — runs the pairing and Groth16 verification code of csrc/pairing.cuh ON THE CPU, driven over stdin/stdout by
// tests/test_pairing_host.py, which checks every result against oracle/groth16_verify_oracle.py. The build container has no GPU: this is
// how the tower, the Miller loop, the final exponentiation and the per-proof check are verified before they run on one. The same source
// is compiled: __device__ is defined away below (every function becomes a host function) and the MAC is the compiler-scheduled one
// (ZKMI_MUL_VARIANT 1) instead of the inline v_mad_u64_u32.
//
// build: hipcc --offload-arch=gfx950 --cuda-host-only -O0 -std=c++17 -Isnarkjs_amd/csrc tools/pairing_hosttest.hip -o tools/bin/pairing_hosttest
// protocol: one request per line "<op> <curve 0|1> <hex integers...>", one reply line of hex integers (or "ERR ...").
//   consts c                          -> g1[0..5], g2[0..5] (Fq2: c0 c1 each), twist_b (c0 c1), b, hard exponent
//   mul|sqr|inv|frob1|frob2 c a[12] [b[12]]   Fq12 in the oracle's w-basis -> 12 coefficients
//   pair c P(x y z) Q(x0 x1 y0 y1 z0 z1)      -> reduced pairing e(P, Q), 12 coefficients
//   verify c n_ic n_sig alpha(3) beta(6) gamma(6) delta(6) IC(3 n_ic) A(3) B(6) C(3) pubs(n_sig) -> verdict code
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
    Fp<C> std_fp() { Words w = parse_hex(tok.at(at++), N); Fp<C> r; for (int i = 0; i < N; i++) r.l[i] = w[i]; return r; }
    void words(Words& out, int count) { for (int k = 0; k < count; k++) { Fp<C> v = std_fp(); out.insert(out.end(), v.l, v.l + N); } }
    std::string out_fp(const Fp<C>& m) { Fp<C> s = fp_from_mont(m); return hex(s.l, N); }
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
        if (op == "consts") {
            std::string s;
            for (int k = 0; k < 6; k++) s += out_fp(K.g1[k].c0) + " " + out_fp(K.g1[k].c1) + " ";
            for (int k = 0; k < 6; k++) s += out_fp(K.g2[k].c0) + " " + out_fp(K.g2[k].c1) + " ";
            return s + out_fp(K.twist_b.c0) + " " + out_fp(K.twist_b.c1) + " " + out_fp(K.b) + " " + hex(K.hard, 48);
        }
        if (op == "mul") { Fp12<C> a = f12_in(), b = f12_in(); return f12_out(f12_mul(a, b)); }
        if (op == "sqr") return f12_out(f12_sqr(f12_in()));
        if (op == "inv") return f12_out(f12_inv(f12_in()));
        if (op == "frob1") return f12_out(f12_frob(f12_in(), K.g1, true));
        if (op == "frob2") return f12_out(f12_frob(f12_in(), K.g2, false));
        if (op == "pair") {
            Words p, q;
            words(p, 3); words(q, 6);
            Fp<C> o[12];
            pairing_one(p.data(), q.data(), &K, o);
            std::string s;
            for (int k = 0; k < 12; k++) s += (k ? " " : "") + hex(o[k].l, N);
            return s;
        }
        if (op == "verify") {
            const uint32_t n_ic = (uint32_t)std::stoul(tok.at(at++)), n_sig = (uint32_t)std::stoul(tok.at(at++));
            Words al, be, ga, de, ic, rec, pubs;
            words(al, 3); words(be, 6); words(ga, 6); words(de, 6); words(ic, 3 * n_ic); words(rec, 12);
            for (uint32_t j = 0; j < n_sig; j++) { Words w = parse_hex(tok.at(at++), 8); pubs.insert(pubs.end(), w.begin(), w.end()); }
            constexpr int NL = miller_lines<C>();
            std::vector<Line<C>> tb(NL), tg(NL), td(NL);
            std::vector<Fp<C>> icm(2 * n_ic + 2);
            Fp12<C> mab;
            const uint32_t flags = vk_prepare(al.data(), be.data(), ga.data(), de.data(), ic.data(), n_ic, &K, icm.data(), tb.data(), tg.data(), td.data(), &mab);
            VkView<C> vk{icm.data(), n_ic, tg.data(), td.data(), flags & 1u, (flags >> 1) & 1u, &mab};
            return std::to_string(groth16_verify_one(rec.data(), pubs.data(), n_sig, vk, &K));
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
