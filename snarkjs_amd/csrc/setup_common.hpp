// snarkjs_amd/csrc/setup_common.hpp — what the two setups (groth16_setup.hip, plonk_setup.hip) share on the host: the device memory of one call,
// a sequential reader over a paged buffer (the r1cs constraint section) and the byte total of a paged buffer.
#pragma once
#include <string.h>
#include <algorithm>
#include <vector>
#include "zkmi_common.hpp"

namespace zkmi {

namespace {                                       // internal to each of the two units, as they were in groth16_setup.hip

struct DevMem {                                   // device memory of one call: freed on every return path
    const char* const who;                        // the entry point's name, the prefix of its error text
    std::vector<void*> blocks;
    explicit DevMem(const char* w) : who(w) {}
    ~DevMem() { for (void* p : blocks) (void)hipFree(p); }
    int get(size_t bytes, void** out) {
        *out = nullptr;
        hipError_t e = hipMalloc(out, bytes ? bytes : 16);
        if (e != hipSuccess) return fail(ZKMI_ERR_HIP, std::string(who) + ": hipMalloc: " + hipGetErrorString(e));
        blocks.push_back(*out);
        return ZKMI_OK;
    }
};

// sequential reader over a paged buffer
struct PageReader {
    const zkmi_pages& pg;
    int page = 0;
    size_t off = 0;
    explicit PageReader(const zkmi_pages& p) : pg(p) {}
    bool read(void* dst, size_t n) {
        uint8_t* d = (uint8_t*)dst;
        while (n) {
            while (page < pg.n_pages && off == pg.len[page]) { page++; off = 0; }
            if (page >= pg.n_pages) return false;
            const size_t k = std::min(n, pg.len[page] - off);
            if (d) { memcpy(d, pg.ptr[page] + off, k); d += k; }
            off += k; n -= k;
        }
        return true;
    }
    bool u32(uint32_t& v) { return read(&v, 4); }
    bool skip(size_t n) { return read(nullptr, n); }
};
inline size_t pages_bytes(const zkmi_pages& p) {
    size_t t = 0;
    for (int i = 0; i < p.n_pages; i++) t += p.len[i];
    return t;
}

}  // namespace

}  // namespace zkmi
