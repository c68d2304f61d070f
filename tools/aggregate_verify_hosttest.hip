// tools/aggregate_verify_hosttest.hip — runs the aggregated check of csrc/kzg_aggregate.cuh and the chain final exponentiation of csrc/pairing.cuh
// ON THE CPU, driven over stdin/stdout by tests/test_aggregate_verify_host.py, which checks every result against the oracles. The same source is
// compiled as for the device: __device__ is defined away below and the MAC is the compiler-scheduled one (ZKMI_MUL_VARIANT 1), exactly as
// tools/plonk_verify_hosttest.hip does. The lanes of a batch run one after the other and their pairs are added in order (the device adds them
// by a tree; the group law makes the sums the same points).
//
// build: hipcc --offload-arch=gfx950 --cuda-host-only -O0 -std=c++17 -Isnarkjs_amd/csrc tools/aggregate_verify_hosttest.hip -o tools/bin/aggregate_verify_hosttest
// protocol: one request per line "<op> <curve 0|1> ...", one reply line (or "ERR ..."). An Fq12 value is twelve Fq coefficients of the oracle's w-basis.
//   x c                                  -> |x| and the G1 cofactor as the code derives them (hex)
//   miller c P (x y z) Q (x0 x1 y0 y1 z0 z1) -> the Miller value of the pair (not reduced)
//   easy | fexp | chain | sqr | cyclo c f -> f^((p^6-1)(p^2+1)) | final_exp(f) | final_exp_chain(f) | f12_sqr(f) | f12_cyclo_sqr(f)
//   isone c f                            -> f12_is_one(final_exp(f)) f12_is_one(final_exp_chain(f))
//   challenge c seed(64 hex digits, the bytes in order) i -> r_i (hex)
//   plonk c power n_public omega_mont k1 k2 Qm..S3 (8 x (x y z)) X_2 (6) seed n { A..Wxiw (9 x (x y z)) evals (6) pubs (n_public) } x n
//   fflonk c power n_public omega_mont k1 k2 w3 w4 w8 wr C0 (x y z) X_2 (6) seed n { C1 C2 W1 W2 (4 x (x y z)) evals (15) pubs (n_public) } x n
//                                        -> ok pair_ok S_P.x S_P.y S_Q.x S_Q.y code_0 .. code_(n-1)
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
#include "plonk_verify.cuh"
#include "fflonk_verify.cuh"
#include "kzg_aggregate.cuh"

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
    void seed_in(uint64_t* w) {
        const std::string h = tok.at(at++);
        if (h.size() != 64) throw std::runtime_error("seed: 64 hex digits");
        uint8_t b[32];
        for (int i = 0; i < 32; i++) b[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
        memcpy(w, b, 32);
    }
    // the batch after the key: lanes in order, the sums, the tail
    template <class Points> std::string aggregate(const Line<C>* tab0, const Line<C>* tab1, bool use0, bool use1, int rec_fq, int rec_fr, uint32_t n_public, Points points) {
        uint64_t seed[4];
        seed_in(seed);
        const size_t n = std::stoul(tok.at(at++));
        AggPair<C> S;
        pt_set_inf(S.p);
        pt_set_inf(S.q);
        std::string codes;
        bool all = true;
        for (size_t i = 0; i < n; i++) {
            Words rec, pubs;
            words(rec, rec_fq, N); words(rec, rec_fr, 8); words(pubs, n_public, 8);
            pubs.resize(pubs.size() + 8);
            KzgPair<C> pr;
            const int code = points(rec.data(), pubs.data(), &pr);
            if (code == AGG_ENTERED) {
                uint64_t lo, hi;
                agg_challenge(seed, i, lo, hi);
                S.p = pt_add(S.p, agg_scale<C>(pr.px, pr.py, pr.p_fin, lo, hi));
                S.q = pt_add(S.q, agg_scale<C>(pr.qx, pr.qy, pr.q_fin, lo, hi));
            }
            all = all && code == AGG_ENTERED;
            codes += " " + std::to_string(code);
        }
        AggResult<C> res;
        memset(&res, 0, sizeof res);
        res.pair_ok = 1;
        if (n) agg_tail(S, tab0, tab1, use0, use1, &K, &res);
        return std::to_string((all && res.pair_ok) ? 1 : 0) + " " + std::to_string(res.pair_ok) + " " + hex(res.sp, N) + " " + hex(res.sp + N, N) + " " + hex(res.sq, N) + " " +
               hex(res.sq + N, N) + codes;
    }
    std::string run(const std::string& op) {
        if (op == "x") {
            constexpr unsigned __int128 H = g1_cofactor<C>();
            const uint32_t x[2] = {(uint32_t)curve_x_abs<C>(), (uint32_t)(curve_x_abs<C>() >> 32)};
            const uint32_t h[4] = {(uint32_t)H, (uint32_t)(H >> 32), (uint32_t)(H >> 64), (uint32_t)(H >> 96)};
            return hex(x, 2) + " " + hex(h, 4);
        }
        if (op == "miller") {
            Words p, q;
            words(p, 3, N); words(q, 6, N);
            Affine<Fp<C>> P;
            Affine<Fp2<C>> Q;
            if (decode_point(p.data(), P) || decode_point(q.data(), Q)) throw std::runtime_error("a point at infinity");
            const FixedPair<C> none{nullptr, P.x, P.y, false};
            return f12_out(miller_multi(Q, fp_neg(P.x), P.y, true, none, none, &K));
        }
        if (op == "easy") {
            const Fp12<C> f = f12_in();
            const Fp12<C> t = f12_mul(f12_conj(f), f12_inv(f));
            return f12_out(f12_mul(f12_frob(t, K.g2, false), t));
        }
        if (op == "fexp") return f12_out(final_exp(f12_in(), &K));
        if (op == "chain") return f12_out(final_exp_chain(f12_in(), &K));
        if (op == "sqr") return f12_out(f12_sqr(f12_in()));
        if (op == "cyclo") return f12_out(f12_cyclo_sqr(f12_in()));
        if (op == "isone") {
            const Fp12<C> f = f12_in();
            return std::to_string((int)f12_is_one(final_exp(f, &K))) + " " + std::to_string((int)f12_is_one(final_exp_chain(f, &K)));
        }
        if (op == "challenge") {
            uint64_t seed[4], lo, hi;
            seed_in(seed);
            agg_challenge(seed, std::stoull(tok.at(at++)), lo, hi);
            const uint32_t r[4] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
            return hex(r, 4);
        }
        if (op == "plonk") {
            const uint32_t power = (uint32_t)std::stoul(tok.at(at++)), n_public = (uint32_t)std::stoul(tok.at(at++));
            Words om, k1, k2, g1, x2;
            words(om, 1, 8); words(k1, 1, 8); words(k2, 1, 8); words(g1, 24, N); words(x2, 6, N);
            constexpr int NL = miller_lines<C>();
            std::vector<Line<C>> tx(NL), tg(NL);
            PlonkVk<C> vk;
            plonk_vk_prepare(g1.data(), x2.data(), k1.data(), k2.data(), om.data(), power, n_public, &K, &vk, tx.data(), tg.data());
            if (vk.bad) throw std::runtime_error("key point not on the curve");
            const PlonkVkView<C> V{&vk, tx.data(), tg.data()};
            return aggregate(tx.data(), tg.data(), !vk.x2_inf, true, 27, 6, n_public,
                             [&](const uint32_t* rec, const uint32_t* pubs, KzgPair<C>* pr) { return plonk_verify_one<C, true>(rec, pubs, V, &K, (PlonkTrace<C>*)nullptr, pr); });
        }
        if (op == "fflonk") {
            if (N != 8) throw std::runtime_error("FFLONK verification serves BN254 only");
            const uint32_t power = (uint32_t)std::stoul(tok.at(at++)), n_public = (uint32_t)std::stoul(tok.at(at++));
            Words om, consts, c0, x2;
            words(om, 1, 8); words(consts, 6, 8); words(c0, 3, N); words(x2, 6, N);
            constexpr int NL = miller_lines<C>();
            std::vector<Line<C>> tx(NL), tg(NL);
            FflonkVk<C> vk;
            fflonk_vk_prepare(c0.data(), x2.data(), consts.data(), om.data(), power, n_public, &K, &vk, tx.data(), tg.data());
            if (vk.bad) throw std::runtime_error("X_2 not on the curve");
            const FflonkVkView<C> V{&vk, tx.data(), tg.data()};
            return aggregate(tg.data(), tx.data(), true, !vk.x2_inf, 12, FFLONK_EVALS, n_public,
                             [&](const uint32_t* rec, const uint32_t* pubs, KzgPair<C>* pr) { return fflonk_verify_one<C, true>(rec, pubs, V, &K, (FflonkTrace<C>*)nullptr, pr); });
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
