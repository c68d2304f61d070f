// tools/ptau_lagrange_hosttest.hip — the lane maps of csrc/ptau_lagrange.cuh as a host program: the functions the three kernels of the Lagrange ladder
// call to find their points, enumerated on the CPU. It needs no device and no library: the host pass of the headers alone.
//   hipcc --offload-arch=gfx950 --cuda-host-only -O1 -std=c++17 -Isnarkjs_amd/csrc tools/ptau_lagrange_hosttest.hip -o tools/bin/ptau_lagrange_hosttest
// (add -Xarch_host -fsanitize=address,undefined for a run under the host sanitizers: the program has its own main).
//   ptau_lagrange_hosttest check <max top>     for every top = 0 .. max top, first in {0, top} and every stage: each butterfly of each block p >= max(st, first)
//                                              is produced exactly once, hi - lo = 2^(st-1) with both inside the block, the twiddle exponent is j << (top - st) for
//                                              the j of lo, idle lanes name no butterfly, and a 64-aligned wave holds one twiddle whenever 2^(top-st+1) >= 64; the
//                                              load writes every point of every block once, from its own source index, and the store lane of a point states its p.
//                                              Prints "ok <butterflies seen>", or the first difference and exits 1.
//   ptau_lagrange_hosttest dump <top> <first>  the maps as text, one lane per line, for a check written in another language:
//                                              "P tid p i dst" for every load / store lane, "S st t idle p j lo hi e" for every stage lane
// The per-lane arithmetic (pt_add, pt_mul_naf on the 32-bit limbs of curve.cuh) is __device__ only and is not run here.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "ptau_lagrange.cuh"

using namespace zkmi;

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); return -1; } while (0)

static long check_one(uint32_t top, uint32_t first) {
    const uint32_t pts = lag_points(first, top);
    long seen_total = 0;
    // load and store
    std::vector<uint8_t> written(pts, 0);
    uint32_t want_tid = 0;
    for (uint32_t p = first; p <= top; p++)
        for (uint32_t i = 0; i < (1u << p); i++, want_tid++) {
            const LagPoint q = lag_point_of(want_tid, first);
            if (q.p != p || q.i != i) FAIL("top %u first %u: lane %u is point (%u, %u), not (%u, %u)", top, first, want_tid, q.p, q.i, p, i);
            const uint32_t dst = lag_load_dst(q, first), base = lag_block_base(p, first);
            if (base != want_tid - i) FAIL("top %u first %u: block %u starts at %u, not %u", top, first, p, base, want_tid - i);
            if (dst < base || dst >= base + (1u << p)) FAIL("top %u first %u: the load of (%u, %u) leaves its block", top, first, p, i);
            if (lag_bitrev(dst - base, p) != i) FAIL("top %u first %u: the load of (%u, %u) is not bit-reversed", top, first, p, i);
            if (written.at(dst)++) FAIL("top %u first %u: place %u is loaded twice", top, first, dst);
        }
    if (want_tid != pts) FAIL("top %u first %u: %u points, not %u", top, first, want_tid, pts);
    for (uint32_t d = 0; d < pts; d++) if (!written[d]) FAIL("top %u first %u: place %u is never loaded", top, first, d);
    // stages
    for (uint32_t st = 1; st <= top; st++) {
        std::vector<uint8_t> lo_seen(pts, 0);
        const uint32_t slots = 1u << (top - st + 1), h = 1u << (st - 1);
        long seen = 0, idle = 0;
        for (uint32_t t = 0; t < (1u << top); t++) {
            const LagButterfly b = lag_stage_lane(t, st, first, top);
            if (t % 64 == 0 && slots >= 64 && lag_stage_lane(t + 63, st, first, top).j != b.j) FAIL("top %u st %u: the wave at lane %u holds two twiddles", top, st, t);
            if (b.j != t / slots) FAIL("top %u st %u: lane %u holds twiddle %u", top, st, t, b.j);
            if (b.idle) { idle++; if (b.lo || b.hi || b.e) FAIL("top %u st %u: idle lane %u names a butterfly", top, st, t); continue; }
            if (b.p < st || b.p < first || b.p > top) FAIL("top %u first %u st %u: lane %u works on block %u", top, first, st, t, b.p);
            const uint32_t base = lag_block_base(b.p, first);
            if (b.hi - b.lo != h || b.lo < base || b.hi >= base + (1u << b.p)) FAIL("top %u first %u st %u: lane %u leaves its block", top, first, st, t);
            if (((b.lo - base) & (2 * h - 1)) != b.j || b.j >= h) FAIL("top %u first %u st %u: lane %u: lo is not at index j of its group", top, first, st, t);
            if (b.e != ((uint64_t)b.j << (top - st))) FAIL("top %u first %u st %u: lane %u: twiddle exponent", top, first, st, t);
            if (lo_seen.at(b.lo)++ || lo_seen.at(b.hi)++) FAIL("top %u first %u st %u: point %u or %u is in two butterflies", top, first, st, b.lo, b.hi);
            seen++;
        }
        long want = 0;
        for (uint32_t p = (st > first ? st : first); p <= top; p++) want += 1l << (p - 1);
        if (seen != want) FAIL("top %u first %u st %u: %ld butterflies, not %ld", top, first, st, seen, want);
        // every point of every block p >= max(st, first) is in a butterfly, no other point is
        for (uint32_t p = first; p <= top; p++)
            for (uint32_t i = 0; i < (1u << p); i++)
                if (lo_seen[lag_block_base(p, first) + i] != (p >= st ? 1 : 0)) FAIL("top %u first %u st %u: point %u of block %u", top, first, st, i, p);
        if (seen + idle != (1l << top)) FAIL("top %u st %u: lanes", top, st);
        seen_total += seen;
    }
    return seen_total;
}

static int dump(uint32_t top, uint32_t first) {
    for (uint32_t tid = 0; tid < lag_points(first, top); tid++) {
        const LagPoint q = lag_point_of(tid, first);
        printf("P %u %u %u %u\n", tid, q.p, q.i, lag_load_dst(q, first));
    }
    for (uint32_t st = 1; st <= top; st++)
        for (uint32_t t = 0; t < (1u << top); t++) {
            const LagButterfly b = lag_stage_lane(t, st, first, top);
            printf("S %u %u %d %u %u %u %u %llu\n", st, t, b.idle ? 1 : 0, b.p, b.j, b.lo, b.hi, (unsigned long long)b.e);
        }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "check")) {
        const uint32_t max_top = (uint32_t)strtoul(argv[2], nullptr, 10);
        if (max_top > 20) { fprintf(stderr, "max top <= 20\n"); return 2; }
        long total = 0;
        for (uint32_t top = 0; top <= max_top; top++)
            for (uint32_t first : {0u, top}) {
                const long n = check_one(top, first);
                if (n < 0) return 1;
                total += n;
                if (!top) break;
            }
        printf("ok %ld\n", total);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "dump")) {
        const uint32_t top = (uint32_t)strtoul(argv[2], nullptr, 10), first = (uint32_t)strtoul(argv[3], nullptr, 10);
        if (top > 12 || first > top) { fprintf(stderr, "first <= top <= 12\n"); return 2; }
        return dump(top, first);
    }
    fprintf(stderr, "usage: ptau_lagrange_hosttest check <max top> | dump <top> <first>\n");
    return 2;
}
