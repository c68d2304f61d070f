"""Which MSM kernel runs (csrc/msm_select.hpp), on the CPU: tools/msm_select_hosttest.hip compiles the two pure pick functions for the host and this
file compares them, over the full product of their inputs and of the switch settings, with a restatement of the rules written from the host driver
as it was before the selection was pulled out of it (csrc/msm_host.hpp: msm_accumulate, msm_reduce). The headline configurations are also spelled
out by name. A second test checks that msm_tuning() parses the eight environment variables as the driver always did. No GPU needed."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "bin", "msm_select_hosttest")
SRC = os.path.join(ROOT, "tools", "msm_select_hosttest.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "snarkjs_amd", "csrc")

UNSUPPORTED, INVALID = 4, 2                     # include/zkmi.h
# the switches in the order of MsmTuning, with their defaults
NAMES = ["ZKMI_ROWCOL_WAVE", "ZKMI_R29_REDUCE", "ZKMI_R29_REDUCE_G2", "ZKMI_ACC29_BLOCK", "ZKMI_G2_SPLIT", "ZKMI_G2_SPLIT_BLS", "ZKMI_AUX_RC_SUMS", "ZKMI_MULTI_OVERLAP"]
DEFAULT = dict(wave=1, r29=1, r29_g2=1, acc_block=0, split=1, split_bls=1, aux_cap=512, overlap=1)
# all at their defaults, then each flipped alone
TUNINGS = [dict(DEFAULT)] + [dict(DEFAULT, **{k: v}) for k, v in (("wave", 0), ("r29", 0), ("r29_g2", 0), ("acc_block", 64), ("acc_block", 128), ("acc_block", 7), ("split", 0),
                                                                  ("split_bls", 0), ("aux_cap", 0), ("aux_cap", 64), ("overlap", 0))]


@pytest.fixture(scope="module")
def tool():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    deps = [SRC, os.path.join(CSRC, "msm_select.hpp"), os.path.join(ROOT, "include", "zkmi.h")]
    if not os.path.exists(TOOL) or any(os.path.getmtime(d) > os.path.getmtime(TOOL) for d in deps):
        os.makedirs(os.path.dirname(TOOL), exist_ok=True)
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O0", "-std=c++17", "-I" + CSRC, SRC, "-o", TOOL])

    def ask(lines, env=None):
        """one process for all the requests; every answer split into fields, the message (it has blanks) joined again as the last one"""
        r = subprocess.run([TOOL], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=60, env=env)
        assert r.returncode == 0, r.stderr
        out = r.stdout.splitlines()
        assert len(out) == len(lines) and not any(o.startswith("ERR") for o in out)
        return out
    return ask


def fields(t):
    return " ".join(str(t[k]) for k in DEFAULT)


def wide_block(limbs):
    """threads of every Fq2 kernel that parks its accumulators in LDS (msm.cuh: MsmAccumBlock — 128 where an Fq2 element has more than 16 words)"""
    return 128 if limbs == 14 else 256


def want_accum(group, limbs, table29, merge, into_r29, c, cc, t):
    """(kernel, threads, lanes per block, dynamic LDS, R'-form buckets) or (error code, message): msm_accumulate of the parent commit, restated"""
    wave_c = (c - 1) // 2 >= 6
    if group == 2:
        if merge:
            return UNSUPPORTED, "msm_accumulate: merge mode is implemented for G1 only"
        T = wide_block(limbs)
        if not table29:
            return "accum32_wide", T, T, 1, 0
        r29 = int(bool(t["wave"] and t["r29_g2"] and not (cc & 8) and wave_c))
        if t["split"] and not (limbs == 14 and not t["split_bls"]):
            return "accum29_g2s", 256, 128, 0, r29
        return ("accum29_g2_compact" if limbs == 14 and cc & 2 else "accum29_g2"), T, T, 1, r29
    if table29:
        T = t["acc_block"] if t["acc_block"] in (64, 128, 256) else (128 if limbs == 14 else 256)
        r29 = into_r29 if merge else int(bool(t["r29"] and t["wave"] and wave_c))
        k = "accum29" + ("_compact" if limbs == 14 and cc & 1 else "") + ("_merge" if merge else "")
        return k, T, T, 0, r29
    if merge and into_r29:
        return INVALID, "msm_accumulate: merge target holds R'-form buckets"
    return ("accum32_merge" if merge else "accum32"), 256, 256, 0, 0


def want_rowcol(group, limbs, all_r29, rbits, cbits, aux, cc, t):
    """(kernel, threads, cap on the blocks or -1, bit sums by k_msm_bitsums_lds) or (error code, message): msm_reduce of the parent commit, restated"""
    wave = bool(t["wave"] and rbits >= 6 and cbits >= 6)
    lds = int(group == 2 and bool(t["wave"]))
    if all_r29 and not wave:
        return UNSUPPORTED, "msm_reduce: R'-form buckets need the wave row/column sums"
    if not wave:
        return "staged", 256, -1, lds
    if all_r29 and group == 1:
        k, T, per = ("wave29_compact" if limbs == 14 and cc & 4 else "wave29"), 256, 4
    else:
        T = wide_block(limbs) if group == 2 else 256
        k, per = ("wave29_g2" if all_r29 else "wave"), T // 64
    return k, T, (t["aux_cap"] // per if aux and t["aux_cap"] > 0 else -1), lds


def check(got_line, want, what):
    if isinstance(want[0], int):                 # a refusal: code and text, nothing else is looked at
        f = got_line.split(" ", 5 if what[0] == "rowcol" else 6)
        assert (int(f[-2]), f[-1]) == want, (what, got_line)
    else:
        f = got_line.split()
        assert (f[0],) + tuple(int(x) for x in f[1:len(want)]) == want and int(f[len(want)]) == 0 and len(f) == len(want) + 1, (what, got_line, want)


def test_accum_pick_full_product(tool):
    cases = [(g, l, tb, m, ir, c, cc, t) for g, l, tb, m, ir, c, cc in itertools.product((1, 2), (9, 14), (0, 1), (0, 1), (0, 1), (12, 13, 15), (0, 14, 31)) for t in TUNINGS]
    got = tool(["accum %d %d %d %d %d %d %d %s" % (x[:7] + (fields(x[7]),)) for x in cases])
    for x, line in zip(cases, got):
        check(line, want_accum(*x), ("accum",) + x)


def test_rowcol_pick_full_product(tool):
    cases = [(g, l, a, rb, cb, aux, cc, t) for g, l, a, rb, cb, aux, cc in itertools.product((1, 2), (9, 14), (0, 1), (5, 6, 7), (5, 6, 7), (0, 1), (0, 14, 31)) for t in TUNINGS]
    got = tool(["rowcol %d %d %d %d %d %d %d %s" % (x[:7] + (fields(x[7]),)) for x in cases])
    for x, line in zip(cases, got):
        check(line, want_rowcol(*x), ("rowcol",) + x)


def test_headline_configurations(tool):
    """what the default configuration runs, by name (resident window tables, c = 15: rbits = cbits = 7)"""
    d = fields(DEFAULT)
    acc = lambda group, limbs, cc: tool(["accum %d %d 1 0 0 15 %d %s" % (group, limbs, cc, d)])[0].split()
    rc = lambda group, limbs, r29, cc: tool(["rowcol %d %d %d 7 7 0 %d %s" % (group, limbs, r29, cc, d)])[0].split()
    # kernel, threads, lanes per block, LDS, R'-form buckets, no error
    assert acc(1, 9, 0) == ["accum29", "256", "256", "0", "1", "0"]                  # BN254 G1: k_msm_accum29<C, false>
    assert acc(1, 14, 0) == ["accum29", "128", "128", "0", "1", "0"]                 # BLS12-381 G1: the same in 128-thread blocks
    assert acc(2, 9, 0) == ["accum29_g2s", "256", "128", "0", "1", "0"]              # both G2 tables: one Fq2 component per lane
    assert acc(2, 14, 0) == ["accum29_g2s", "256", "128", "0", "1", "0"]
    assert rc(1, 9, 1, 0)[:2] == ["wave29", "256"] and rc(1, 14, 1, 0)[:2] == ["wave29", "256"]
    assert rc(2, 9, 1, 0)[:2] == ["wave29_g2", "256"] and rc(2, 14, 1, 0)[:2] == ["wave29_g2", "128"]
    # a slow-fetch box (compact_code 14) on BLS12-381: G1 accumulation still the plain one, G2 still split but its buckets back in R-form (so the generic
    # wave sums reduce them), the G1 row / column sums by the Compact instantiation
    assert acc(1, 14, 14) == ["accum29", "128", "128", "0", "1", "0"]
    assert acc(2, 14, 14) == ["accum29_g2s", "256", "128", "0", "0", "0"]
    assert rc(1, 14, 1, 14)[:2] == ["wave29_compact", "256"]
    assert rc(2, 14, 0, 14)[:2] == ["wave", "128"]
    # BN254 has no Compact instantiation whatever the box says
    assert acc(1, 9, 31)[0] == "accum29" and rc(1, 9, 1, 31)[0] == "wave29"


def test_tuning_from_the_environment(tool):
    """msm_tuning(): defaults with nothing set; a boolean switch is off only when set and atoi() of it is 0; the two numbers are taken as they are
    (the pick, not the parser, ignores a block size other than 64 / 128 / 256)"""
    clean = {k: v for k, v in os.environ.items() if not k.startswith("ZKMI_")}
    env = lambda *vals: dict(clean, **dict(zip(NAMES, vals)))
    assert tool(["env"], env=clean) == ["1 1 1 0 1 1 512 1"]
    assert tool(["env"], env=env("0", "0", "0", "64", "0", "0", "0", "0")) == ["0 0 0 64 0 0 0 0"]
    assert tool(["env"], env=env("1", "2", "-1", "7", "1", "1", "64", "1")) == ["1 1 1 7 1 1 64 1"]
    assert tool(["env"], env=env("", "off", "00", "128", "x", " 0", "-5", "no")) == ["0 0 0 128 0 0 -5 0"]
    for i, name in enumerate(NAMES):             # one variable at a time: no switch reads another's name
        want = ["1", "1", "1", "0", "1", "1", "512", "1"]
        want[i] = "0"
        assert tool(["env"], env=dict(clean, **{name: "0"})) == [" ".join(want)]
