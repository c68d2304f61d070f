// tools/chacha_hosttest.hip — the generator of csrc/chacha.cuh as a host program: the block function and the attempt rule the kernels run, held to the
// sequential generator struct and field_from_rng of csrc/phase2_host.hpp. It needs no device and no library: the host pass of the headers alone.
//   hipcc --offload-arch=gfx950 --cuda-host-only -O1 -std=c++17 -Isnarkjs_amd/csrc tools/chacha_hosttest.hip -o tools/bin/chacha_hosttest
// (add -Xarch_host -fsanitize=address,undefined for a run under the host sanitizers: the program has its own main).
//   chacha_hosttest <seed word 0> .. <seed word 7> <draws>
// checks, for both curves: the keystream by blocks against the struct from counter 0 and from counter 2^32 - 2 (the carry out of word 12), the first
// <draws> kept attempts and the position against sequential draws. Prints "ok <words bn254> <words bls12381>", or the first difference and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "field.cuh"
#define ZKMI_CHACHA_NO_KERNELS
#include "chacha.cuh"
#include "phase2_host.hpp"

using namespace zkmi;

static int keystream(const uint32_t* seed, uint64_t first_block) {
    phase2::ChaCha rng(seed);
    rng.state[12] = (uint32_t)first_block; rng.state[13] = (uint32_t)(first_block >> 32);
    for (uint64_t b = first_block; b < first_block + 5; b++) {
        uint32_t w[16];
        chacha::block(seed, b, 0, w);
        for (int i = 0; i < 16; i++)
            if (w[i] != rng.next_u32()) { printf("block %llu word %d differs\n", (unsigned long long)b, i); return 1; }
    }
    return 0;
}

template <class FrC> static int draws(const uint32_t* seed, size_t n, uint64_t* words) {
    const host::HField<4> Fr = host::HField<4>::from_cfg<FrC>();
    std::vector<uint8_t> got(32 * n + 1);
    *words = chacha::fr_stream_host<FrC>(seed, got.data(), n);
    phase2::ChaCha rng(seed);
    for (size_t i = 0; i < n; i++) {
        const host::HFp<4> v = phase2::field_from_rng(Fr, rng);
        if (memcmp(got.data() + 32 * i, v.v, 32)) { printf("draw %zu differs\n", i); return 1; }
    }
    const uint64_t blocks = ((uint64_t)rng.state[13] << 32) | rng.state[12];
    const uint64_t at = n ? 16 * blocks - (16 - (uint64_t)rng.idx) : 0;
    if (at != *words) { printf("position %llu, sequential %llu\n", (unsigned long long)*words, (unsigned long long)at); return 1; }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 10) { fprintf(stderr, "usage: chacha_hosttest s0 .. s7 draws\n"); return 2; }
    uint32_t seed[8];
    for (int i = 0; i < 8; i++) seed[i] = (uint32_t)strtoul(argv[1 + i], nullptr, 10);
    const size_t n = (size_t)strtoull(argv[9], nullptr, 10);
    if (keystream(seed, 0) || keystream(seed, 0xfffffffeull)) return 1;
    uint64_t w0 = 0, w1 = 0;
    if (draws<Bn254Fr>(seed, n, &w0) || draws<Bls12381Fr>(seed, n, &w1)) return 1;
    printf("ok %llu %llu\n", (unsigned long long)w0, (unsigned long long)w1);
    return 0;
}
