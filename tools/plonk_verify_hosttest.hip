// tools/plonk_verify_hosttest.hip — runs the PLONK verification code of csrc/plonk_verify.cuh ON THE CPU, driven over stdin/stdout by
// tests/test_plonk_verify_host.py, which checks every result against oracle/plonk_verify_oracle.py and the pairing oracle. The same source
// is compiled as for the device: __device__ is defined away below and the MAC is the compiler-scheduled one (ZKMI_MUL_VARIANT 1), exactly as
// tools/pairing_hosttest.hip does for pairing.cuh.
//
// build: hipcc --offload-arch=gfx950 --cuda-host-only -O0 -std=c++17 -Isnarkjs_amd/csrc tools/plonk_verify_hosttest.hip -o tools/bin/plonk_verify_hosttest
// protocol: one request per line "<op> <curve 0|1> ...", one reply line (or "ERR ...").
//   keccak c <hex bytes | ->                                  -> the digest, hex bytes
//   verify c power n_public omega_mont k1 k2 Qm..S3 (8 x (x y z)) X_2 (x0 x1 y0 y1 z0 z1) A..Wxiw (9 x (x y z)) evals (6) pubs (n_public)
//                                                             -> code beta gamma alpha xi v1 u L1 PI r0 A1.x A1.y B1.x B1.y   (hex integers)
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

// Keccak-256 of any byte string through the verifier's own sponge: whole 8-byte lanes go through keccak_lane (the absorb path of the
// transcript), and a message that ends on a lane boundary — all the verifier ever hashes — is padded and read out by keccak_finish. Only a
// ragged tail, which no transcript has, is padded here.
static void keccak_any(const uint8_t* data, size_t len, uint8_t* out32) {
    Keccak256 k;
    keccak_init(k);
    size_t i = 0;
    for (; i + 8 <= len; i += 8) { uint64_t w; memcpy(&w, data + i, 8); keccak_lane(k, w); }
    if (i == len) {
        uint32_t d[8];                                       // the digest as a big-endian integer in little-endian words
        keccak_finish(k, d);
        for (int j = 0; j < 32; j++) out32[j] = (uint8_t)(d[(31 - j) / 4] >> (8 * ((31 - j) % 4)));
        return;
    }
    uint64_t w = 0;
    memcpy(&w, data + i, len - i);
    k.st[k.pos] ^= w ^ (0x01ull << (8 * (len - i)));
    k.st[16] ^= 0x8000000000000000ull;
    keccak_f1600(k.st);
    for (int j = 0; j < 32; j++) out32[j] = (uint8_t)(k.st[j >> 3] >> (8 * (j & 7)));
}

template <class C> struct Run {
    static constexpr int N = C::N;
    PairingConsts<C> K;
    std::vector<std::string> tok;
    size_t at = 0;
    Run() { pairing_consts_host(K); }
    void words(Words& out, int count, int nw) { for (int k = 0; k < count; k++) { Words w = parse_hex(tok.at(at++), nw); out.insert(out.end(), w.begin(), w.end()); } }
    std::string run(const std::string& op) {
        if (op == "keccak") {
            const std::string h = tok.at(at++);
            std::vector<uint8_t> msg;
            if (h != "-")
                for (size_t i = 0; i + 1 < h.size(); i += 2) msg.push_back((uint8_t)std::stoul(h.substr(i, 2), nullptr, 16));
            uint8_t out[32];
            keccak_any(msg.data(), msg.size(), out);
            char buf[65];
            for (int i = 0; i < 32; i++) snprintf(buf + 2 * i, 3, "%02x", out[i]);
            return buf;
        }
        if (op == "verify") {
            const uint32_t power = (uint32_t)std::stoul(tok.at(at++)), n_public = (uint32_t)std::stoul(tok.at(at++));
            Words om, k1, k2, g1, x2, rec, pubs;
            words(om, 1, 8); words(k1, 1, 8); words(k2, 1, 8); words(g1, 24, N); words(x2, 6, N); words(rec, 27, N); words(rec, 6, 8); words(pubs, n_public, 8);
            pubs.resize(pubs.size() + 8);
            constexpr int NL = miller_lines<C>();
            std::vector<Line<C>> tx(NL), tg(NL);
            PlonkVk<C> vk;
            plonk_vk_prepare(g1.data(), x2.data(), k1.data(), k2.data(), om.data(), power, n_public, &K, &vk, tx.data(), tg.data());
            if (vk.bad) throw std::runtime_error("key point not on the curve");
            PlonkVkView<C> V{&vk, tx.data(), tg.data()};
            PlonkTrace<C> tr;
            memset(&tr, 0, sizeof tr);
            const int code = plonk_verify_one(rec.data(), pubs.data(), V, &K, &tr);
            std::string s = std::to_string(code);
            for (int j = 0; j < 9; j++) s += " " + hex(tr.fr[j], 8);
            return s + " " + hex(tr.a1, N) + " " + hex(tr.a1 + N, N) + " " + hex(tr.b1, N) + " " + hex(tr.b1 + N, N);
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
