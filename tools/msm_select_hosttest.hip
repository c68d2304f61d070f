// tools/msm_select_hosttest.hip — the MSM kernel selection (csrc/msm_select.hpp) as a host program for tests/test_msm_select_host.py.
// One request per line on stdin, one answer per line on stdout. The switches are fields of the line (in the order of MsmTuning), not
// environment variables, so one process serves every case:
//   accum  group limbs table29 merge into_r29 c compact_code  <8 switches>  ->  kernel threads lanes_per_block lds r29_buckets code [message]
//   rowcol group limbs all_r29 rbits cbits aux compact_code   <8 switches>  ->  kernel threads max_blocks(-1: none) bitsums_lds code [message]
//   env                                                                     ->  the 8 fields of msm_tuning(), read from this process's environment
// and with the lanes per row / column sum (the answers above stay as they were):
//   rowcol_lanes group limbs all_r29 rbits cbits aux compact_code n_sums  <8 switches> rc_lanes rc_lanes_g2
//                                                                           ->  kernel threads max_blocks bitsums_lds lanes code [message]
//   env_lanes                                                               ->  rc_lanes rc_lanes_g2 of msm_tuning()
#include <stdio.h>
#include <string.h>
#include "msm_select.hpp"

using namespace zkmi;

static const char* ACCUM[] = {"accum29", "accum29_merge", "accum29_compact", "accum29_compact_merge", "accum29_g2s", "accum29_g2", "accum29_g2_compact",
                              "accum32", "accum32_merge", "accum32_wide"};
static const char* ROWCOL[] = {"wave29", "wave29_compact", "wave29_g2", "wave", "staged"};

static MsmTuning tuning(const int* v) {
    MsmTuning t;
    t.rowcol_wave = v[0]; t.r29_reduce = v[1]; t.r29_reduce_g2 = v[2]; t.acc29_block = v[3];
    t.g2_split = v[4]; t.g2_split_bls = v[5]; t.aux_rc_sums = v[6]; t.multi_overlap = v[7];
    return t;
}

int main() {
    char line[512], op[16];
    while (fgets(line, sizeof line, stdin)) {
        int v[18], n = 0, used = 0;
        if (sscanf(line, "%15s%n", op, &used) != 1) continue;
        for (const char* p = line + used; n < 18; n++) {
            int adv = 0;
            if (sscanf(p, "%d%n", &v[n], &adv) != 1) break;
            p += adv;
        }
        if (!strcmp(op, "env")) {
            const MsmTuning& e = msm_tuning();
            printf("%d %d %d %d %d %d %d %d\n", e.rowcol_wave, e.r29_reduce, e.r29_reduce_g2, e.acc29_block, e.g2_split, e.g2_split_bls, e.aux_rc_sums, e.multi_overlap);
        } else if (!strcmp(op, "accum") && n == 15) {
            const MsmAccumPick p = msm_accum_pick(v[0], v[1], v[2], v[3], v[4], v[5], v[6], tuning(v + 7));
            printf("%s %u %u %d %d %d %s\n", ACCUM[(int)p.kernel], p.threads, p.lanes_per_block, p.lds, p.r29_buckets, msm_pick_code(p.error), msm_pick_message(p.error));
        } else if (!strcmp(op, "rowcol") && n == 15) {
            const MsmRowcolPick p = msm_rowcol_pick(v[0], v[1], v[2], (uint32_t)v[3], (uint32_t)v[4], v[5], v[6], tuning(v + 7));
            printf("%s %u %lld %d %d %s\n", ROWCOL[(int)p.kernel], p.threads, p.max_blocks == SIZE_MAX ? -1ll : (long long)p.max_blocks, p.bitsums_lds, msm_pick_code(p.error),
                   msm_pick_message(p.error));
        } else if (!strcmp(op, "env_lanes")) {
            printf("%d %d\n", msm_tuning().rc_lanes, msm_tuning().rc_lanes_g2);
        } else if (!strcmp(op, "rowcol_lanes") && n == 18) {
            MsmTuning t = tuning(v + 8);
            t.rc_lanes = v[16]; t.rc_lanes_g2 = v[17];
            const MsmRowcolPick p = msm_rowcol_pick(v[0], v[1], v[2], (uint32_t)v[3], (uint32_t)v[4], v[5], v[6], t, (size_t)v[7]);
            printf("%s %u %lld %d %u %d %s\n", ROWCOL[(int)p.kernel], p.threads, p.max_blocks == SIZE_MAX ? -1ll : (long long)p.max_blocks, p.bitsums_lds, p.lanes,
                   msm_pick_code(p.error), msm_pick_message(p.error));
        } else printf("ERR bad request\n");
        fflush(stdout);
    }
    return 0;
}
