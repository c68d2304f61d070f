// tools/ptau_challenge_hosttest.hip — the per-lane routines of the per-lane-scalar G2 multiplication (csrc/ptau_challenge.cuh: mul_each_point29_g2, the body of
// k_group2_mul_each, then scale_affine_group29_g2, the body of k_group2_scale_affine) as a host program. It needs no device and no library: the host pass of
// the header alone.
//   hipcc --offload-arch=gfx950 --cuda-host-only -O1 -std=c++17 -DZK29_CHECK -DZK29_BOUNDS -Isnarkjs_amd/csrc tools/ptau_challenge_hosttest.hip -o tools/bin/ptau_challenge_hosttest
// (add -fsanitize=address,undefined for a run under the host sanitizers: the program has its own main). -DZK29_CHECK makes every lazy subtraction check
// its offset exactly, -DZK29_BOUNDS carries worst-case bounds through every product (field29.cuh); a violated bound fails the request it shows up in.
// One request per line on stdin, one answer per line on stdout (tests/test_ptau_challenge_kernel_host.py):
//   <bn254|bls12381|bls12381_compact> <scalars: 32 bytes each as hex, little-endian, normal form> <points: 4 N words each as hex, the reference's bytes>
// with as many scalars as points ("-" for none). The points go through exactly what a grid of the two kernels does: every point through mul_each_point29_g2
// into a work array, its accumulator parked in an "LDS" array of one lane in the kernel's own layout (packed words for the 12-word field), then groups of
// SCALE_INV through scale_affine_group29_g2, the last group short, into a SEPARATE output array. Answer: the affine points as hex, or ERR and a reason.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "ptau_challenge.cuh"

using namespace zkmi;

static int hexval(char c) { return c >= '0' && c <= '9' ? c - '0' : (c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1); }

template <class C> static std::string run(const std::vector<uint8_t>& sc, const std::vector<uint8_t>& in) {
    constexpr int N = C::N;
    typedef LdsAcc29<C, 1, Reduce29G2<C>::PACK> Acc;                 // one lane: stride 1
    const size_t n = in.size() / (4 * N * 4);
    // 16-byte aligned like device memory, and exactly as long as the kernels may touch
    uint32_t* src = (uint32_t*)aligned_alloc(16, (n ? n : 1) * 4 * N * 4);
    uint32_t* k = (uint32_t*)aligned_alloc(16, (n ? n : 1) * 32);
    uint32_t* work = (uint32_t*)aligned_alloc(16, (n ? n : 1) * 8 * N * 4);
    uint32_t* dst = (uint32_t*)aligned_alloc(16, (n ? n : 1) * 4 * N * 4);
    uint32_t* lds = (uint32_t*)aligned_alloc(16, 8 * Acc::EW * 4);
    if (n) { memcpy(src, in.data(), n * 4 * N * 4); memcpy(k, sc.data(), n * 32); }
    for (size_t i = 0; i < n; i++) {
#if defined(ZK29_SHADOW)
        b29::parked().clear();                                             // a lane starts with nothing parked
#endif
        mul_each_point29_g2<C>(Acc{lds}, src + i * 4 * N, k + i * 8, work + i * 8 * N);
    }
    for (size_t i0 = 0; i0 < n; i0 += SCALE_INV) scale_affine_group29_g2<C>(work + i0 * 8 * N, dst + i0 * 4 * N, (uint32_t)(n - i0 < (size_t)SCALE_INV ? n - i0 : SCALE_INV));
    std::string out;
    char b[3];
    for (size_t i = 0; i < n * 4 * N * 4; i++) { snprintf(b, sizeof b, "%02x", ((const uint8_t*)dst)[i]); out += b; }
    free(src); free(k); free(work); free(dst); free(lds);
    return out.empty() ? "-" : out;
}

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

int main() {
    std::string line;
    char buf[1 << 16];
    while (fgets(buf, sizeof buf, stdin)) {
        line = buf;
        while (!line.empty() && line.back() != '\n' && fgets(buf, sizeof buf, stdin)) line += buf;
        while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
        const size_t a = line.find(' '), b = a == std::string::npos ? a : line.find(' ', a + 1);
        if (b == std::string::npos) { printf("ERR request\n"); fflush(stdout); continue; }
        const std::string curve = line.substr(0, a);
        std::vector<uint8_t> sc, pts;
        const bool ok = unhex(line.substr(a + 1, b - a - 1), sc) && unhex(line.substr(b + 1), pts);
        const bool bn = curve == "bn254", bls = curve == "bls12381", blc = curve == "bls12381_compact";
        const size_t sG = bn ? 128 : 192;
        if (!ok || !(bn || bls || blc) || pts.size() % sG || sc.size() != pts.size() / sG * 32) { printf("ERR argument\n"); fflush(stdout); continue; }
#if defined(ZK29_SHADOW)
        const int before = b29::failures();
#endif
        const std::string out = bn ? run<Bn254Fq>(sc, pts) : (bls ? run<Bls12381Fq>(sc, pts) : run<Compact<Bls12381Fq>>(sc, pts));
#if defined(ZK29_SHADOW)
        if (b29::failures() != before) { printf("ERR %d bounds violated\n", b29::failures() - before); fflush(stdout); continue; }
#endif
        printf("%s\n", out.c_str());
        fflush(stdout);
    }
    return 0;
}
