// tools/bellman_hosttest.hip — the per-lane routines of the Bellman H basis change (csrc/bellman.cuh: the bodies of k_bellman_import_load, k_bellman_export_twist
// and k_bellman_export_store) as a host program. It needs no device and no library: the host pass of the header alone.
//   hipcc --offload-arch=gfx950 --cuda-host-only -O1 -std=c++17 -DZK29_CHECK -DZK29_BOUNDS -Isnarkjs_amd/csrc tools/bellman_hosttest.hip -o tools/bin/bellman_hosttest
// (add -Xarch_host -fsanitize=address,undefined for a run under the host sanitizers: the program has its own main). -DZK29_CHECK makes every lazy subtraction
// check its offset exactly, -DZK29_BOUNDS carries worst-case bounds through every product (field29.cuh); a violated bound fails the request it shows up in.
// One request per line on stdin, one answer per line on stdout (tests/test_bellman_kernel_host.py):
//   <bn254|bls12381|bls12381_compact> <log_n> <k1: n - 1 scalars> <k2: n - 1 scalars> <n - 1 uncompressed points>          n = 2^log_n
// scalars 32 bytes each as hex, little-endian, normal form; points as the reference's big-endian bytes. The points go through what grids of the three kernels
// do with the butterflies left out: slot i of bellman_import_slot29 for every i < n (work[bitrev(i)] = k1_i P_i, the last slot infinity), then
// bellman_export_point29 in place on work[j] with k2_j for j < n - 1, then groups of SCALE_INV through bellman_affine_u_group29, the last group short, into a
// separate output array. Answer: the n - 1 uncompressed points k2_j k1_bitrev(j) P_bitrev(j) as hex, a space, and the 4 N words of work[n - 1] as hex (the
// slot of the dropped coefficient: all zero); or ERR and a reason.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "bellman.cuh"

using namespace zkmi;

static int hexval(char c) { return c >= '0' && c <= '9' ? c - '0' : (c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1); }

// R'^2 mod p by doubling: 2^(2 B NL)
template <class C> static BellmanRR<C::N> rr_host() {
    constexpr int N = C::N;
    BellmanRR<N> v;
    memset(v.w, 0, sizeof v.w);
    v.w[0] = 1;
    for (int s = 0; s < 2 * Lim29<C>::B * Lim29<C>::NL; s++) {
        uint32_t carry = 0;
        for (int i = 0; i < N; i++) { const uint32_t t = v.w[i]; v.w[i] = (t << 1) | carry; carry = t >> 31; }
        bool ge = carry != 0;
        if (!ge) { ge = true; for (int i = N - 1; i >= 0; i--) if (v.w[i] != C::p(i)) { ge = v.w[i] > C::p(i); break; } }
        if (ge) { uint64_t bw = 0; for (int i = 0; i < N; i++) { const uint64_t d = (uint64_t)v.w[i] - C::p(i) - bw; v.w[i] = (uint32_t)d; bw = (d >> 32) & 1u; } }
    }
    return v;
}

static std::string hex_of(const void* p, size_t n) {
    std::string out;
    char b[3];
    for (size_t i = 0; i < n; i++) { snprintf(b, sizeof b, "%02x", ((const uint8_t*)p)[i]); out += b; }
    return out;
}

template <class C> static std::string run(uint32_t log_n, const std::vector<uint8_t>& k1, const std::vector<uint8_t>& k2, const std::vector<uint8_t>& in) {
    constexpr int N = C::N;
    const uint32_t n = 1u << log_n, m = n - 1;
    const BellmanRR<N> rr = rr_host<C>();
    // 16-byte aligned like device memory, and exactly as long as the kernels may touch
    uint32_t* src = (uint32_t*)aligned_alloc(16, (size_t)m * 2 * N * 4);
    uint32_t* s1 = (uint32_t*)aligned_alloc(16, (size_t)m * 32);
    uint32_t* s2 = (uint32_t*)aligned_alloc(16, (size_t)m * 32);
    uint32_t* work = (uint32_t*)aligned_alloc(16, (size_t)n * 4 * N * 4);
    uint32_t* dst = (uint32_t*)aligned_alloc(16, (size_t)m * 2 * N * 4);
    memcpy(src, in.data(), (size_t)m * 2 * N * 4); memcpy(s1, k1.data(), (size_t)m * 32); memcpy(s2, k2.data(), (size_t)m * 32);
    memset(work, 0xa5, (size_t)n * 4 * N * 4);
    for (uint32_t i = 0; i < n; i++) bellman_import_slot29<C>(src, s1, rr, work, i, n, log_n);
    for (uint32_t j = 0; j < m; j++) bellman_export_point29<C>(work + (size_t)j * 4 * N, s2 + (size_t)j * 8);
    for (uint32_t i0 = 0; i0 < m; i0 += SCALE_INV) bellman_affine_u_group29<C>(work + (size_t)i0 * 4 * N, dst + (size_t)i0 * 2 * N, m - i0 < (uint32_t)SCALE_INV ? m - i0 : (uint32_t)SCALE_INV);
    const std::string out = hex_of(dst, (size_t)m * 2 * N * 4) + " " + hex_of(work + (size_t)m * 4 * N, (size_t)4 * N * 4);
    free(src); free(s1); free(s2); free(work); free(dst);
    return out;
}

static bool unhex(const std::string& s, std::vector<uint8_t>& out) {
    if (s.size() % 2) return false;
    for (size_t i = 0; i < s.size(); i += 2) {
        const int a = hexval(s[i]), b = hexval(s[i + 1]);
        if (a < 0 || b < 0) return false;
        out.push_back((uint8_t)(a * 16 + b));
    }
    return true;
}

int main() {
    std::string line;
    static char buf[1 << 16];
    while (fgets(buf, sizeof buf, stdin)) {
        line = buf;
        while (!line.empty() && line.back() != '\n' && fgets(buf, sizeof buf, stdin)) line += buf;
        while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
        std::vector<std::string> f;
        for (size_t at = 0; at <= line.size();) { const size_t sp = line.find(' ', at); f.push_back(line.substr(at, sp == std::string::npos ? sp : sp - at)); if (sp == std::string::npos) break; at = sp + 1; }
        if (f.size() != 5) { printf("ERR request\n"); fflush(stdout); continue; }
        const std::string& curve = f[0];
        const long log_n = strtol(f[1].c_str(), nullptr, 10);
        std::vector<uint8_t> k1, k2, pts;
        const bool ok = unhex(f[2], k1) && unhex(f[3], k2) && unhex(f[4], pts);
        const bool bn = curve == "bn254", bls = curve == "bls12381", blc = curve == "bls12381_compact";
        const size_t sG = bn ? 64 : 96;
        if (!ok || !(bn || bls || blc) || log_n < 1 || log_n > 12 || pts.size() != (((size_t)1 << log_n) - 1) * sG || k1.size() != pts.size() / sG * 32 || k2.size() != k1.size()) {
            printf("ERR argument\n"); fflush(stdout); continue;
        }
#if defined(ZK29_SHADOW)
        const int before = b29::failures();
#endif
        const std::string out = bn ? run<Bn254Fq>((uint32_t)log_n, k1, k2, pts) : (bls ? run<Bls12381Fq>((uint32_t)log_n, k1, k2, pts) : run<Compact<Bls12381Fq>>((uint32_t)log_n, k1, k2, pts));
#if defined(ZK29_SHADOW)
        if (b29::failures() != before) { printf("ERR %d bounds violated\n", b29::failures() - before); fflush(stdout); continue; }
#endif
        printf("%s\n", out.c_str());
        fflush(stdout);
    }
    return 0;
}
