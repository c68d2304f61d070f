// snarkjs_amd/csrc/r1cs_host.hpp — the host passes of the witness check (r1cs_check.hip) that need no device: the offset pass over r1cs section 2 and the
// rule that cuts a batch of witnesses. Plain C++ over zkmi_pages, so that a host program can test them (tools/r1cs_check_hosttest.hip).
//
// r1cs section 2 (r1csfile): per constraint three linear combinations A, B, C, each u32 n then n x (u32 signal, 32-byte little-endian coefficient). With
// lc_first[l] = number of terms before combination l (l = 3 * constraint + matrix), term t of combination l lies at byte 4 * (l + 1) + 36 * (lc_first[l] + t):
// l + 1 counts and lc_first[l] + t records precede it. Every offset is a multiple of 4.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/zkmi.h"

namespace zkmi {

enum { R1CS_OFFSETS_OK = 0, R1CS_OFFSETS_SHORT = 1, R1CS_OFFSETS_TOO_MANY = 2 };

// Reads only the 3 * n_constraints term counts. lc_first gets 3 * n_constraints + 1 entries (the last one: all terms); *used = the bytes the constraints
// take. SHORT: the section ends inside a count or a record (nothing past the end is read). TOO_MANY: 2^32 terms or more. Bytes after the last constraint
// are left alone. A page may end anywhere, inside a count or a record.
inline int r1cs_lc_offsets(const zkmi_pages& pg, uint32_t n_constraints, std::vector<uint32_t>& lc_first, uint64_t* used) {
    const uint64_t n_lc = 3ull * n_constraints;
    lc_first.assign((size_t)n_lc + 1, 0u);
    int page = 0;
    size_t off = 0;                                  // position inside the current page
    uint64_t terms = 0, pos = 0;
    auto settle = [&]() { while (page < pg.n_pages && off == pg.len[page]) { page++; off = 0; } return page < pg.n_pages; };
    auto skip = [&](uint64_t n) {
        while (n) {
            if (!settle()) return false;
            const uint64_t k = n < (uint64_t)(pg.len[page] - off) ? n : (uint64_t)(pg.len[page] - off);
            off += (size_t)k; n -= k;
        }
        return true;
    };
    auto u32 = [&](uint32_t& v) {
        uint8_t b[4];
        for (int i = 0; i < 4; i++) {
            if (!settle()) return false;
            b[i] = pg.ptr[page][off++];
        }
        v = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
        return true;
    };
    for (uint64_t l = 0; l < n_lc; l++) {
        uint32_t n = 0;
        lc_first[(size_t)l] = (uint32_t)terms;
        if (!u32(n) || !skip(36ull * n)) return R1CS_OFFSETS_SHORT;
        terms += n; pos += 4 + 36ull * n;
        if (terms >> 32) return R1CS_OFFSETS_TOO_MANY;
    }
    lc_first[(size_t)n_lc] = (uint32_t)terms;
    if (used) *used = pos;
    return R1CS_OFFSETS_OK;
}

// How many witnesses one pass of the check takes: as many as fit `budget` bytes of per-witness work memory (per_witness bytes each: the reduced witness,
// the 3 * n_constraints evaluations and the partial sums), at least one, at most `limit` (the grid's second dimension) and no more than there are.
inline uint32_t r1cs_batch_cut(uint64_t per_witness, uint32_t n_witnesses, uint64_t budget, uint32_t limit) {
    if (n_witnesses == 0) return 0;
    uint64_t k = per_witness ? budget / per_witness : n_witnesses;
    if (k > limit) k = limit;
    if (k > n_witnesses) k = n_witnesses;
    return k ? (uint32_t)k : 1u;
}

}  // namespace zkmi
