// tools/group_scale_hosttest.hip — the per-lane routines of the one-scalar point scaling (csrc/group_scale.cuh: scale_point29, the body of k_group_scale,
// and scale_affine_group29, the body of k_group_scale_affine) as a host program. It needs no device and no library: the host pass of the header alone.
//   hipcc --offload-arch=gfx950 --cuda-host-only -O1 -std=c++17 -DZK29_CHECK -DZK29_BOUNDS -Isnarkjs_amd/csrc tools/group_scale_hosttest.hip -o tools/bin/group_scale_hosttest
// (add -fsanitize=address,undefined for a run under the host sanitizers: the program has its own main). -DZK29_CHECK makes every lazy subtraction check
// its offset exactly, -DZK29_BOUNDS carries worst-case bounds through every product (field29.cuh); a violated bound fails the request it shows up in.
// One request per line on stdin, one answer per line on stdout (tests/test_group_scale_host.py):
//   <bn254|bls12381|bls12381_compact> k <k as 64 hex digits, a plain integer, most significant first> <points: 2 N words each as hex, the reference's bytes>
//   <curve> d <digits, most significant first, one of + - 0 each>  <points>       a raw digit stream: it need not be a non-adjacent form nor stay below r
// The points go through exactly what a grid of the two kernels does: every point through scale_point29 into a work array, then groups of SCALE_INV through
// scale_affine_group29, the last group short. Answer: the affine points as hex, or ERR and a reason.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "group_scale.cuh"

using namespace zkmi;

static int hexval(char c) { return c >= '0' && c <= '9' ? c - '0' : (c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1); }

template <class C> static std::string run(const ScaleDigits& d, const std::vector<uint8_t>& in) {
    constexpr int N = C::N;
    const size_t n = in.size() / (2 * N * 4);
    // 16-byte aligned like device memory, and exactly as long as the kernels may touch
    uint32_t* src = (uint32_t*)aligned_alloc(16, (n ? n : 1) * 2 * N * 4);
    uint32_t* work = (uint32_t*)aligned_alloc(16, (n ? n : 1) * 4 * N * 4);
    if (n) memcpy(src, in.data(), n * 2 * N * 4);
    for (size_t i = 0; i < n; i++) scale_point29<C>(src + i * 2 * N, work + i * 4 * N, d);
    for (size_t i0 = 0; i0 < n; i0 += SCALE_INV) scale_affine_group29<C>(work + i0 * 4 * N, src + i0 * 2 * N, (uint32_t)(n - i0 < (size_t)SCALE_INV ? n - i0 : SCALE_INV));   // in place, as d_out == d_in
    std::string out;
    char b[3];
    for (size_t i = 0; i < n * 2 * N * 4; i++) { snprintf(b, sizeof b, "%02x", ((const uint8_t*)src)[i]); out += b; }
    free(src); free(work);
    return out.empty() ? "-" : out;
}

int main() {
    std::string line;
    char buf[1 << 16];
    while (fgets(buf, sizeof buf, stdin)) {
        line = buf;
        while (!line.empty() && line.back() != '\n' && fgets(buf, sizeof buf, stdin)) line += buf;
        char curve[32], kind[4];
        int used = 0;
        if (sscanf(line.c_str(), "%31s %3s %n", curve, kind, &used) < 2) { printf("ERR request\n"); fflush(stdout); continue; }
        const char* p = line.c_str() + used;
        const char* sp = strchr(p, ' ');
        const std::string arg(p, sp ? (size_t)(sp - p) : strlen(p));
        ScaleDigits d;
        memset(&d, 0, sizeof d);
        bool ok = true;
        if (kind[0] == 'k') {
            uint64_t k[4] = {0, 0, 0, 0};
            ok = arg.size() == 64;
            for (size_t i = 0; ok && i < 64; i++) { const int v = hexval(arg[63 - i]); ok = v >= 0; k[i / 16] |= (uint64_t)(v & 15) << (4 * (i % 16)); }
            if (ok) d = scale_recode(k);
        } else {
            ok = arg.size() <= (size_t)SCALE_MAX_DIGITS;
            for (size_t j = 0; ok && j < arg.size(); j++) {
                const uint32_t t = arg[j] == '+' ? 1u : (arg[j] == '-' ? 3u : 0u);
                ok = arg[j] == '+' || arg[j] == '-' || arg[j] == '0';
                d.w[j >> 4] |= t << (2 * (j & 15));
            }
            d.n = (uint32_t)arg.size();
        }
        std::vector<uint8_t> pts;
        for (const char* q = sp ? sp + 1 : ""; ok && hexval(q[0]) >= 0 && hexval(q[1]) >= 0; q += 2) pts.push_back((uint8_t)(hexval(q[0]) * 16 + hexval(q[1])));
        const bool bn = !strcmp(curve, "bn254"), bls = !strcmp(curve, "bls12381"), blc = !strcmp(curve, "bls12381_compact");
        if (!ok || !(bn || bls || blc) || pts.size() % (bn ? 64 : 96)) { printf("ERR argument\n"); fflush(stdout); continue; }
#if defined(ZK29_SHADOW)
        const int before = b29::failures();
#endif
        const std::string out = bn ? run<Bn254Fq>(d, pts) : (bls ? run<Bls12381Fq>(d, pts) : run<Compact<Bls12381Fq>>(d, pts));
#if defined(ZK29_SHADOW)
        if (b29::failures() != before) { printf("ERR %d bounds violated\n", b29::failures() - before); fflush(stdout); continue; }
#endif
        printf("%s\n", out.c_str());
        fflush(stdout);
    }
    return 0;
}
