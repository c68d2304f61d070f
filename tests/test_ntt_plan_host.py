"""How the Fr NTT driver cuts a transform into passes (csrc/ntt_plan.hpp: ntt_split, the function get_plan and ntt_run decide with), on the CPU, through the
host-only probe zkmi_ntt_plan_probe (include/zkmi_diag.h). The switches are read once per process, so every setting is asked in a child process of its own.
The expected splits are restated here from the rule (ceil(log_n / cap) digits whose widths differ by at most one, the wider ones first) and the headline
ones spelled out. This pins that tests/test_gpu_ntt_passes.py reaches the four-pass path it claims to reach: a changed digit cap fails here instead of
silently turning its cases back into three passes. No GPU needed."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, INVALID = 4, 2                     # include/zkmi.h
FR_S = {0: 28, 1: 32}                           # 2-adicity of r - 1: BN254, BLS12-381
MAX_PASSES, TILE_LOG = 4, 9                     # csrc/ntt_plan.hpp
SENTINEL = [77, [9, 9, 9, 9], -5]               # what the outputs hold before a call: a refusal leaves them alone

CHILD = (
    "import sys, json, ctypes as C; sys.path.insert(0, %r)\n"
    "from snarkjs_amd import zkmi\n"
    "L, out = zkmi.lib(), {}\n"
    "for c in (0, 1):\n"
    "    for lg in range(0, 35):\n"
    "        n, l, f = C.c_uint32(77), (C.c_uint32 * 4)(9, 9, 9, 9), C.c_int(-5)\n"
    "        rc = L.zkmi_ntt_plan_probe(c, lg, C.byref(n), l, C.byref(f))\n"
    "        out['%%d:%%d' %% (c, lg)] = [rc, n.value, list(l), f.value, L.zkmi_last_error().decode() if rc else '']\n"
    "out['null'] = L.zkmi_ntt_plan_probe(0, 9, None, None, None)\n"
    "out['curve'] = L.zkmi_ntt_plan_probe(2, 9, None, None, None)\n"
    "print('PLAN ' + json.dumps(out))\n") % ROOT


def ask(**env):
    """the probe's answers for both curves and every log_n in a fresh process with only the given ZKMI_NTT* switches set"""
    clean = {k: v for k, v in os.environ.items() if not k.startswith("ZKMI_NTT")}
    r = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=120, env=dict(clean, **env))
    assert r.returncode == 0, r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("PLAN ")]
    assert len(line) == 1, r.stdout[-2000:]
    d = json.loads(line[0][5:])
    assert d.pop("null") == 0 and d.pop("curve") == INVALID          # every output is optional; an unknown curve is refused
    return {tuple(int(x) for x in k.split(":")): v for k, v in d.items()}


def want_split(lg, cap):
    """the rule, restated: None where the driver has to refuse"""
    if lg <= TILE_LOG:
        return [lg]
    if not 1 <= cap <= TILE_LOG or -(-lg // cap) > MAX_PASSES:
        return None
    p, out = -(-lg // cap), []
    for i in range(p):
        out.append(-(-(lg - sum(out)) // (p - i)))
    return out


def check_all(got, cap, limbs29):
    for (c, lg), (rc, n_pass, l, f29, msg) in got.items():
        want = want_split(lg, cap) if lg <= FR_S[c] else None
        if want is None:
            assert rc == UNSUPPORTED and [n_pass, l, f29] == SENTINEL, (c, lg, rc, n_pass, l, f29)
            if lg > FR_S[c]:
                assert "2-adicity" in msg, msg
            else:                                # the message names the size and the cap
                assert "log_n = %d " % lg in msg and "cap of %d bits" % cap in msg and "ZKMI_NTT_DIGIT" in msg, msg
            continue
        assert rc == 0 and n_pass == len(want) and l == want + [0] * (4 - len(want)), (c, lg, rc, n_pass, l, want)
        assert sum(l) == lg and max(l) - min(want) <= 1 and l[:n_pass] == sorted(want, reverse=True), (c, lg, l)
        assert f29 == int(limbs29(lg)), (c, lg, f29)


def test_default_split_and_limb_form():
    got = ask()
    check_all(got, 8, lambda lg: lg <= 22)
    for c in (0, 1):
        passes = {lg: got[c, lg][1] for lg in range(0, FR_S[c] + 1)}
        assert all(passes[lg] == 1 for lg in range(0, 10))
        assert all(passes[lg] == 2 for lg in range(10, 17))
        assert all(passes[lg] == 3 for lg in range(17, 25))
        assert all(passes[lg] == 4 for lg in range(25, FR_S[c] + 1))
        assert [got[c, lg][2] for lg in (25, 26, 27, 28)] == [[7, 6, 6, 6], [7, 7, 6, 6], [7, 7, 7, 6], [7, 7, 7, 7]]
        assert all(sum(got[c, lg][2]) == lg for lg in range(0, FR_S[c] + 1))
        assert [got[c, lg][3] for lg in (0, 9, 22, 23, 25, 28)] == [1, 1, 1, 0, 0, 0]         # the 29-bit passes up to 2^22
        assert got[c, FR_S[c]][0] == 0 and got[c, FR_S[c] + 1][0] == UNSUPPORTED
    assert got[1, 32][2] == [8, 8, 8, 8]


def test_digit_cap_4_gives_four_passes_and_refuses_17():
    got = ask(ZKMI_NTT_DIGIT="4")
    check_all(got, 4, lambda lg: lg <= 22)
    for c in (0, 1):
        assert [got[c, lg][1:3] for lg in (13, 14, 15, 16)] == [[4, [4, 3, 3, 3]], [4, [4, 4, 3, 3]], [4, [4, 4, 4, 3]], [4, [4, 4, 4, 4]]]
        assert [got[c, lg][1] for lg in (9, 10, 12)] == [1, 3, 3]
        rc, n_pass, l, f29, msg = got[c, 17]
        assert rc == UNSUPPORTED and [n_pass, l, f29] == SENTINEL and "needs 5 passes" in msg and "at most 4" in msg, got[c, 17]


@pytest.mark.parametrize("cap,four", [(3, [10, 11, 12]), (5, [16, 17, 18, 19, 20])])
def test_digit_caps_of_the_gpu_tests(cap, four):
    """the other two settings tests/test_gpu_ntt_passes.py runs: which sizes are four passes, and that some of them have unequal digits"""
    got = ask(ZKMI_NTT_DIGIT=str(cap))
    check_all(got, cap, lambda lg: lg <= 22)
    for c in (0, 1):
        assert [lg for lg in range(0, FR_S[c] + 1) if got[c, lg][0] == 0 and got[c, lg][1] == 4] == four
        assert any(len(set(got[c, lg][2])) > 1 for lg in four)
        assert got[c, four[-1] + 1][0] == UNSUPPORTED


@pytest.mark.parametrize("cap", ["0", "10", "-1", "x"])
def test_digit_cap_without_a_tile_is_refused(cap):
    """a cap of 0 (no digit at all; "x" parses as 0) or above the tile (a digit of more than 9 bits has no tile) is refused for every multi-pass size;
    one-tile sizes do not look at it"""
    got = ask(ZKMI_NTT_DIGIT=cap)
    for c in (0, 1):
        assert all(got[c, lg][:3] == [0, 1, [lg, 0, 0, 0]] for lg in range(0, 10))
        for lg in range(10, FR_S[c] + 1):
            rc, n_pass, l, f29, msg = got[c, lg]
            assert rc == UNSUPPORTED and [n_pass, l, f29] == SENTINEL and "the cap must be 1..9" in msg, got[c, lg]


def test_limb_form_switches():
    check_all(ask(ZKMI_NTT29="1"), 8, lambda lg: True)
    check_all(ask(ZKMI_NTT29="0"), 8, lambda lg: False)
    check_all(ask(ZKMI_NTT29_MAX_LOG="16"), 8, lambda lg: lg <= 16)
    check_all(ask(ZKMI_NTT29="0", ZKMI_NTT_DIGIT="5"), 5, lambda lg: False)
