// snarkjs_amd/csrc/ptau_host.hpp — the host side of powersOfTau.verify (src/powersoftau_verify.js): Blake2b-512 with a state that can be
// restored from the 216 bytes a contribution keeps of its response hash (src/misc.js:89-127), and the equality of two Jacobian points. Plain C++, no device.
#pragma once
#include <stdint.h>
#include <string.h>
#include "host_field.hpp"

namespace zkmi {
namespace ptau {

// Blake2b with a 64-byte digest and no key, kept the way the reference's hasher keeps it: `length` counts every byte taken, `pos` of them lie in the block
// buffer, and a full buffer is compressed only when another byte arrives, so the last block is still there for the final compression.
struct Blake2b512 {
    uint64_t h[8];
    uint8_t buf[128];
    uint64_t length;
    size_t pos;

    static uint64_t iv(int i) {
        static const uint64_t IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                                       0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
        return IV[i];
    }
    Blake2b512() : length(0), pos(0) {
        for (int i = 0; i < 8; i++) h[i] = iv(i);
        h[0] ^= 0x01010040ull;                    // digest length 64, no key, fanout 1, depth 1
        memset(buf, 0, sizeof buf);
    }
    // misc.fromPartialHash: the block buffer, the eight state words as (low, high) pairs of 32-bit words, length - pos in words 16 / 17, pos in 18 / 19.
    // false: a position beyond the buffer, which no hasher writes
    bool restore(const uint8_t* partial216) {
        memcpy(buf, partial216, 128);
        uint32_t w[22];
        memcpy(w, partial216 + 128, 88);
        for (int i = 0; i < 8; i++) h[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
        const uint64_t rest = (uint64_t)w[16] | ((uint64_t)w[17] << 32), p = (uint64_t)w[18] | ((uint64_t)w[19] << 32);
        if (p > 128) return false;
        pos = (size_t)p;
        length = rest + p;
        return true;
    }
    static uint64_t rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }
    void compress(const uint8_t* block, bool last) {
        static const uint8_t SIGMA[12][16] = {
            {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
            {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
            {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
            {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
            {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
            {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};
        uint64_t m[16], v[16];
        memcpy(m, block, 128);
        for (int i = 0; i < 8; i++) { v[i] = h[i]; v[8 + i] = iv(i); }
        v[12] ^= length;                          // the counter's upper 64 bits stay zero: fewer than 2^64 bytes
        if (last) v[14] = ~v[14];
#define ZKMI_B2B_G(a, b, c, d, x, y)                                                       \
    v[a] = v[a] + v[b] + (x); v[d] = rotr(v[d] ^ v[a], 32); v[c] = v[c] + v[d]; v[b] = rotr(v[b] ^ v[c], 24); \
    v[a] = v[a] + v[b] + (y); v[d] = rotr(v[d] ^ v[a], 16); v[c] = v[c] + v[d]; v[b] = rotr(v[b] ^ v[c], 63);
        for (int r = 0; r < 12; r++) {
            const uint8_t* s = SIGMA[r];
            ZKMI_B2B_G(0, 4, 8, 12, m[s[0]], m[s[1]])
            ZKMI_B2B_G(1, 5, 9, 13, m[s[2]], m[s[3]])
            ZKMI_B2B_G(2, 6, 10, 14, m[s[4]], m[s[5]])
            ZKMI_B2B_G(3, 7, 11, 15, m[s[6]], m[s[7]])
            ZKMI_B2B_G(0, 5, 10, 15, m[s[8]], m[s[9]])
            ZKMI_B2B_G(1, 6, 11, 12, m[s[10]], m[s[11]])
            ZKMI_B2B_G(2, 7, 8, 13, m[s[12]], m[s[13]])
            ZKMI_B2B_G(3, 4, 9, 14, m[s[14]], m[s[15]])
        }
#undef ZKMI_B2B_G
        for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[8 + i];
    }
    void update(const uint8_t* data, size_t len) {
        while (len) {
            if (pos == 128) { compress(buf, false); pos = 0; }
            const size_t take = len < 128 - pos ? len : 128 - pos;
            memcpy(buf + pos, data, take);
            pos += take; length += take; data += take; len -= take;
        }
    }
    // One `update` call of the reference's hasher (the Blake2 base class of its bundle), which the block buffer remembers: a full block that more bytes
    // of the SAME call follow is compressed straight from the input and never copied, so the bytes of the buffer beyond `pos` are whatever an earlier
    // copy left there. update() above gives the same digest for any cut of the data but copies every block; misc.toPartialHash writes the whole buffer
    // into the file, so a contribution's 216 bytes need this path. (The reference takes the direct path only for input whose byte offset in its
    // ArrayBuffer is a multiple of 4; its callers pass whole buffers.)
    void update_call(const uint8_t* data, size_t len) {
        size_t c = 0;
        while (c < len) {
            if (pos == 128) { compress(buf, false); pos = 0; }
            const size_t take = len - c < 128 - pos ? len - c : 128 - pos;
            if (take != 128 || !(c + take < len)) {
                memcpy(buf + pos, data + c, take);
                pos += take; length += take; c += take;
            } else {
                for (; c + 128 < len; c += 128) { length += 128; compress(data + c, false); }
            }
        }
    }
    // misc.toPartialHash: the inverse of restore(); words 17 and 19 stay zero and word 16 is length - pos cut to 32 bits, as the reference writes them
    void partial(uint8_t* partial216) const {
        memcpy(partial216, buf, 128);
        uint32_t w[22];
        memset(w, 0, sizeof w);
        for (int i = 0; i < 8; i++) { w[2 * i] = (uint32_t)h[i]; w[2 * i + 1] = (uint32_t)(h[i] >> 32); }
        w[16] = (uint32_t)(length - pos);
        w[18] = (uint32_t)pos;
        memcpy(partial216 + 128, w, 88);
    }
    void digest(uint8_t* out64) {
        memset(buf + pos, 0, 128 - pos);
        compress(buf, true);
        memcpy(out64, h, 64);
    }
};

// G.eq on two Jacobian points: X1 Z2^2 == X2 Z1^2 and Y1 Z2^3 == Y2 Z1^3, infinity (Z == 0) equal to infinity alone
template <class FT> bool jacobian_eq(const host::HCurve<FT>& G, const host::HPoint<FT>& a, const host::HPoint<FT>& b) {
    if (G.is_zero(a) || G.is_zero(b)) return G.is_zero(a) && G.is_zero(b);
    const FT& F = G.F;
    const typename FT::E za2 = F.sqr(a.Z), zb2 = F.sqr(b.Z);
    if (!(F.mul(a.X, zb2) == F.mul(b.X, za2))) return false;
    return F.mul(a.Y, F.mul(zb2, b.Z)) == F.mul(b.Y, F.mul(za2, a.Z));
}

}  // namespace ptau
}  // namespace zkmi
