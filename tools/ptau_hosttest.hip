// tools/ptau_hosttest.hip — csrc/ptau_host.hpp as a host program: Blake2b-512 with a restored state and the equality of Jacobian points. It needs no device
// and no library: the host pass of the headers alone.
//   hipcc --offload-arch=gfx950 --cuda-host-only -O1 -std=c++17 -Isnarkjs_amd/csrc tools/ptau_hosttest.hip -o tools/bin/ptau_hosttest
// (add -Xarch_host -fsanitize=address,undefined for a run under the host sanitizers: the program has its own main).
//   ptau_hosttest <message length>
// checks: the digest of "abc" (RFC 7693, appendix A); for a message of the given length and every cut of it at 0, 1, 127, 128, 129, 255, 256, 257 and
// length - 1 bytes, the state written out as misc.toPartialHash writes it, restored and fed the rest, against the digest of the whole; a position beyond the
// buffer refused; a point against itself at another Z, against its negative and against infinity, on both curves and both groups.
// Prints "ok <digest of the message in hex>", or the first difference and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "field.cuh"
#include "ptau_host.hpp"

using namespace zkmi;

static void to_partial(const ptau::Blake2b512& hs, uint8_t* out216) {
    memset(out216, 0, 216);
    memcpy(out216, hs.buf, 128);
    uint32_t w[22] = {0};
    for (int i = 0; i < 8; i++) { w[2 * i] = (uint32_t)hs.h[i]; w[2 * i + 1] = (uint32_t)(hs.h[i] >> 32); }
    const uint64_t rest = hs.length - hs.pos;
    w[16] = (uint32_t)rest; w[17] = (uint32_t)(rest >> 32); w[18] = (uint32_t)hs.pos;
    memcpy(out216 + 128, w, 88);
}

static int hashes(size_t len, uint8_t* whole) {
    static const uint8_t abc[64] = {0xba, 0x80, 0xa5, 0x3f, 0x98, 0x1c, 0x4d, 0x0d, 0x6a, 0x27, 0x97, 0xb6, 0x9f, 0x12, 0xf6, 0xe9, 0x4c, 0x21, 0x2f, 0x14, 0x68, 0x5a,
                                    0xc4, 0xb7, 0x4b, 0x12, 0xbb, 0x6f, 0xdb, 0xff, 0xa2, 0xd1, 0x7d, 0x87, 0xc5, 0x39, 0x2a, 0xab, 0x79, 0x2d, 0xc2, 0x52, 0xd5, 0xde,
                                    0x45, 0x33, 0xcc, 0x95, 0x18, 0xd3, 0x8a, 0xa8, 0xdb, 0xf1, 0x92, 0x5a, 0xb9, 0x23, 0x86, 0xed, 0xd4, 0x00, 0x99, 0x23};
    uint8_t d[64];
    { ptau::Blake2b512 hs; hs.update((const uint8_t*)"abc", 3); hs.digest(d); }
    if (memcmp(d, abc, 64)) { printf("the digest of abc differs\n"); return 1; }
    std::vector<uint8_t> msg(len ? len : 1);
    for (size_t i = 0; i < len; i++) msg[i] = (uint8_t)(i * 131 + (i >> 8) * 7 + 3);
    { ptau::Blake2b512 hs; hs.update(msg.data(), len); hs.digest(whole); }
    const size_t cuts[] = {0, 1, 127, 128, 129, 255, 256, 257, len ? len - 1 : 0};
    for (size_t cut : cuts) {
        if (cut > len) continue;
        ptau::Blake2b512 first, second;
        first.update(msg.data(), cut);
        uint8_t partial[216];
        to_partial(first, partial);
        if (!second.restore(partial)) { printf("cut %zu: the state was refused\n", cut); return 1; }
        // exactly the remaining bytes, from a buffer of their own: a read beyond them is the sanitizer's to report
        std::vector<uint8_t> rest(msg.begin() + cut, msg.begin() + len);
        second.update(rest.data(), rest.size());
        second.digest(d);
        if (memcmp(d, whole, 64)) { printf("cut %zu: the resumed digest differs\n", cut); return 1; }
    }
    uint8_t bad[216] = {0};
    bad[128 + 4 * 18] = 129;
    ptau::Blake2b512 hs;
    if (hs.restore(bad)) { printf("position 129 was accepted\n"); return 1; }
    return 0;
}

template <class FT> static int points(const FT& F, const typename FT::E& x, const typename FT::E& y, const typename FT::E& k, const char* what) {
    const host::HCurve<FT> G{F};
    typedef host::HPoint<FT> P;
    const P a{x, y, F.One()}, inf = G.zero();
    const typename FT::E k2 = F.sqr(k);
    const P b{F.mul(x, k2), F.mul(y, F.mul(k2, k)), k};
    const P inf2{x, y, F.zero()};                                  // infinity is Z == 0, whatever X and Y hold
    const bool ok = ptau::jacobian_eq(G, a, a) && ptau::jacobian_eq(G, a, b) && ptau::jacobian_eq(G, b, a) && !ptau::jacobian_eq(G, a, G.neg(b)) &&
                    !ptau::jacobian_eq(G, a, P{F.add(x, F.One()), y, F.One()}) && ptau::jacobian_eq(G, inf, inf2) && !ptau::jacobian_eq(G, a, inf) &&
                    !ptau::jacobian_eq(G, inf2, b);
    if (!ok) printf("%s: the equality of Jacobian points is wrong\n", what);
    return ok ? 0 : 1;
}

template <class FqC> static int points_of(const char* g1, const char* g2) {
    constexpr int L = FqC::N / 2;
    const host::HField<L> F = host::HField<L>::template from_cfg<FqC>();
    const host::HField2<L> F2{F};
    const auto e = [&](uint64_t v) { return F.from_u64(v); };
    if (points(F, e(1), e(2), e(0x1234567890abcdefull), g1)) return 1;
    return points(F2, host::HFp2<L>{e(5), e(7)}, host::HFp2<L>{e(11), e(13)}, host::HFp2<L>{e(17), e(0xfedcba9876543211ull)}, g2);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: ptau_hosttest <message length>\n"); return 2; }
    uint8_t whole[64];
    if (hashes((size_t)strtoull(argv[1], nullptr, 10), whole)) return 1;
    if (points_of<Bn254Fq>("bn254 G1", "bn254 G2") || points_of<Bls12381Fq>("bls12-381 G1", "bls12-381 G2")) return 1;
    printf("ok ");
    for (int i = 0; i < 64; i++) printf("%02x", whole[i]);
    printf("\n");
    return 0;
}
