// snarkjs_amd/csrc/ntt_plan.hpp — how the Fr NTT driver (ntt.hip) cuts a transform into passes and which limb form its kernels run: pure host
// code without a device call, shared by get_plan / ntt_run and by the probe zkmi_ntt_plan_probe (include/zkmi_diag.h), so that what a test asks
// the probe is what a transform runs.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string>
#include "../../include/zkmi.h"

namespace zkmi {

constexpr int NTT_MAX_PASSES = 4;
#ifndef ZKMI_NTT_TILE_LOG
#define ZKMI_NTT_TILE_LOG 9
#endif
// 512 elements = 16 KiB of LDS per workgroup -> 8 workgroups (8 waves per SIMD) per CU: the butterflies are latency-bound carry
// chains, occupancy matters more than tile size (2^20 transform: 0.150 ms; 1024-element tiles 0.163 ms; 2048-element tiles 0.180 ms;
// A/B on one box, PLONK's 2^22 transforms unchanged)
constexpr int NTT_TILE_LOG = ZKMI_NTT_TILE_LOG;
constexpr unsigned NTT_DIGIT_DEFAULT = 8;

struct NttSplit {
    int n_pass = 0;
    uint32_t l[NTT_MAX_PASSES] = {0, 0, 0, 0};      // digit widths, l[0] = most significant input digit; they sum to log_n
};

// The digit split: one pass up to 2^NTT_TILE_LOG (a transform that fits one tile), else ceil(log_n / max_bits) passes whose widths differ by at
// most one bit, the wider ones first. With the default cap of 8 bits: 2 passes for 2^10..2^16, 3 for 2^17..2^24, 4 for 2^25..2^32 (2^25 =
// 7,6,6,6; 2^26 = 7,7,6,6; 2^27 = 7,7,7,6; 2^28 = 7,7,7,7). Four is all the kernels' argument block, the plan and the pre-scale tables hold:
// a cap that would need more is refused (ZKMI_ERR_UNSUPPORTED, *err names log_n and the cap), and so is a cap of 0 or above NTT_TILE_LOG (a digit
// of more than NTT_TILE_LOG bits has no tile). Nothing is written to *out on a refusal.
inline int ntt_split(unsigned log_n, unsigned max_bits, NttSplit* out, std::string* err) {
    NttSplit s;
    if (log_n <= (unsigned)NTT_TILE_LOG) { s.n_pass = 1; s.l[0] = log_n; *out = s; return ZKMI_OK; }
    if (max_bits < 1 || max_bits > (unsigned)NTT_TILE_LOG) {
        if (err) *err = "fft: log_n = " + std::to_string(log_n) + " with a digit cap of " + std::to_string(max_bits) + " bits (ZKMI_NTT_DIGIT): the cap must be 1.." + std::to_string(NTT_TILE_LOG);
        return ZKMI_ERR_UNSUPPORTED;
    }
    const unsigned n_pass = (log_n + max_bits - 1) / max_bits;
    if (n_pass > (unsigned)NTT_MAX_PASSES) {
        if (err) *err = "fft: log_n = " + std::to_string(log_n) + " with a digit cap of " + std::to_string(max_bits) + " bits (ZKMI_NTT_DIGIT) needs " + std::to_string(n_pass) +
                        " passes, the driver holds at most " + std::to_string(NTT_MAX_PASSES);
        return ZKMI_ERR_UNSUPPORTED;
    }
    s.n_pass = (int)n_pass;
    unsigned rem = log_n;
    for (unsigned i = 0; i < n_pass; i++) { const unsigned li = (rem + (n_pass - i) - 1) / (n_pass - i); s.l[i] = li; rem -= li; }
    *out = s;
    return ZKMI_OK;
}

// The driver's switches, read from the environment once per process:
//   ZKMI_NTT_DIGIT      the digit cap (default 8)
//   ZKMI_NTT29          1 / 0 forces the 29-bit (ntt29.cuh) / the 32-bit (ntt.cuh) passes for every size
//   ZKMI_NTT29_MAX_LOG  unforced: the 29-bit passes up to this log_n (default 22)
struct NttKnobs { unsigned digit; int env29; unsigned max29; };
inline const NttKnobs& ntt_knobs() {
    static const NttKnobs k = {getenv("ZKMI_NTT_DIGIT") ? (unsigned)atoi(getenv("ZKMI_NTT_DIGIT")) : NTT_DIGIT_DEFAULT, getenv("ZKMI_NTT29") ? atoi(getenv("ZKMI_NTT29")) : -1,
                               getenv("ZKMI_NTT29_MAX_LOG") ? (unsigned)atoi(getenv("ZKMI_NTT29_MAX_LOG")) : 22u};
    return k;
}
// the split and the limb form of a transform of 2^log_n points under this process's switches
inline int ntt_split_env(unsigned log_n, NttSplit* out, std::string* err) { return ntt_split(log_n, ntt_knobs().digit, out, err); }
inline bool ntt_use29(unsigned log_n) { const NttKnobs& k = ntt_knobs(); return k.env29 >= 0 ? k.env29 == 1 : log_n <= k.max29; }

}  // namespace zkmi
