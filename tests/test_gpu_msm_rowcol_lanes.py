"""The row / column sums of the bucket reduction with 8, 16, 32 and 64 lanes per sum (csrc/msm29.cuh: k_msm_rowcol_wave29<C, LPS>, its Compact
instantiation and k_msm_rowcol_wave29_g2<C, LPS>; csrc/msm_select.hpp: msm_rowcol_pick, ZKMI_RC_LANES / ZKMI_RC_LANES_G2), on the device.

The switches are read once per process, so every forced value runs in a child of its own (as tests/test_gpu_msm_reduce.py: test_table_stages_under_switch);
a child forces the same value for both groups and runs one curve and group. It drives zkmi_msm_stage_probe_dev over caller-owned bases with 4-byte scalars
(three bucket sets: the sum index runs over windows too) at the three smallest shapes at which the mapping of lanes to sums can go wrong:
  c = 13  rbits / cbits 6 / 6   64 entries per sum: one per lane at 64 lanes, eight per lane at 8
  c = 14            6 / 7   half of the row slots are empty (i >= R); rows of 128 against columns of 64
  c = 15            7 / 7   square, 128 entries per sum
with the patterns of tests/msm_reduce_patterns.py that tests/test_msm_rowcol_lanes_host.py holds to their purpose for every LPS: constant (a doubling at
every tree level), alternate_fine and alternate_coarse (cancellation, then infinity skipped, inside a group of lanes and inside a lane), one_per_row with
the lone point at place 0, LPS - 1, LPS and the last one, and at c = 13 the two level patterns (a cancellation at every tree level). Buckets, row / column
sums and the folded result are compared exactly through to_affine with arithmetic mod r (test_gpu_msm_reduce.run_case). A batched call of three jobs over
one table goes through the same launch with njobs = 3, and zkmi_msm_rowcol_lanes must report the forced value after every one of them. One case per group
runs the c = 20 table of the headline without a switch: the default pick, and the kernel the info record has always named."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import msm_patterns as P
import msm_reduce_patterns as M
import oracle_lib as O
import test_gpu_msm_reduce as T
import test_msm_rowcol_lanes_host as H

pytestmark = pytest.mark.gpu
ROOT = T.ROOT
KINDS = ("constant", "alternate_fine", "alternate_coarse", "one_per_row")
LEVELS = ("levels_rows", "levels_cols")             # c = 13 only


def terms_of(kind, c, r, lps, sb=4):
    """the pattern in every window that holds scalar bits (the top one as far as it does)"""
    Wd, terms = P.digits_of(sb, c), []
    for w in range(Wd):
        top_bits = 8 * sb - c * w
        if top_bits <= 0:
            continue
        lim = None if top_bits >= c else (1 << top_bits) - 1
        terms += [(w, b, v) for _, b, v in H.pattern(kind, c, r, lps) if lim is None or b < lim]
    return terms, Wd


def batched(lib, name, group, lps):
    """three jobs over one c = 13 table of G and -G (4096 each): every bucket G; G or -G by the parity of row + column; by bit 5 of the column"""
    from snarkjs_amd import zkmi
    cid, r, c = O.CURVE_ID[name], M.order(name), 13
    nb, pj = 1 << (c - 1), 3 * group * O.n8q(cid)
    _, cbits = P.grid_bits(c)
    row, col = np.arange(nb) >> cbits, np.arange(nb) & ((1 << cbits) - 1)
    jobs, want = [], []
    for minus in (np.zeros(nb, bool), (row + col) & 1 == 1, (col >> 5) & 1 == 1):
        s = np.zeros((2 * nb, 8), np.uint32)
        s[:nb, 0] = np.where(minus, 0, np.arange(nb) + 1)
        s[nb:, 0] = np.where(minus, np.arange(nb) + 1, 0)
        want.append(sum((b + 1) * (-1 if m else 1) for b, m in enumerate(minus.tolist())) % r)
        jobs.append(zkmi.DeviceBuffer.from_host(s.view(np.uint8).reshape(-1)))
    d_k = zkmi.DeviceBuffer.from_host(P.logs_bytes([1] * nb + [r - 1] * nb))
    d_b = zkmi.DeviceBuffer(2 * nb * 2 * group * O.n8q(cid))
    h = C.c_uint64(0)
    try:
        zkmi.check(lib.zkmi_gen_bases_from_scalars_dev(cid, group, d_k.ptr, 2 * nb, d_b.ptr))
        zkmi.check(lib.zkmi_msm_table_build(cid, group, d_b.ptr, 2 * nb, C.byref(h)))
        out = np.full(3 * pj, 0xA5, np.uint8)
        zkmi.check(lib.zkmi_msm_table_multi_dev(h, (C.c_void_p * 3)(*[b.ptr for b in jobs]), (C.c_size_t * 3)(*[2 * nb] * 3), 3, 32, zkmi.ptr(out)))
    finally:
        if h.value:
            lib.zkmi_msm_table_release(h)
        for b in jobs + [d_k, d_b]:
            b.free()
    for i, k in enumerate(want):
        jac = out[i * pj:(i + 1) * pj]
        if k == 0:
            assert not jac.any(), i
        else:
            assert np.array_equal(O.to_affine(cid, group, jac), np.frombuffer(T.affine_of(name, group, k), np.uint8)), i
    assert lib.zkmi_msm_rowcol_lanes(group) == lps, (name, group, lps, lib.zkmi_msm_rowcol_lanes(group))


def child_lanes(name, group, lps):
    from snarkjs_amd import zkmi
    zkmi.init(0)
    lib, r = zkmi.lib(), M.order(name)
    assert os.environ["ZKMI_RC_LANES"] == os.environ["ZKMI_RC_LANES_G2"] == str(lps)
    assert lib.zkmi_msm_rowcol_lanes(group) == 0                            # no reduction yet
    want_kernel = T.WAVE29_G2 if group == 2 else T.WAVE29
    for c in (13, 14, 15):
        for kind in KINDS + (LEVELS if c == 13 else ()):
            t0 = time.time()
            terms, Wd = terms_of(kind, c, r, lps)
            try:
                assert lib.zkmi_msm_set_window_bits(c) == 0
                info = T.run_case(name, group, terms, c, Wd, 4)
            finally:
                lib.zkmi_msm_set_window_bits(0)
            assert info["rowcol_kernel"] == want_kernel and info["bitsums"] == 1 and info["W"] == 3, info
            assert lib.zkmi_msm_rowcol_lanes(group) == lps, (c, kind, lib.zkmi_msm_rowcol_lanes(group))
            print("case", name, group, c, kind, json.dumps(info), "%.2f s" % (time.time() - t0), flush=True)
    t0 = time.time()
    batched(lib, name, group, lps)
    print("batched %.2f s" % (time.time() - t0))
    assert lib.zkmi_msm_rowcol_lanes(3 - group) == 0                        # the other group has not reduced anything
    print("lanes ok")


def child_c20(group):
    """BN254, a c = 20 table over 2^19 bases, no switch set: what the headline runs"""
    from snarkjs_amd import zkmi
    assert os.environ["ZKMI_TABLE_C"] == "20" and "ZKMI_RC_LANES" not in os.environ and "ZKMI_RC_LANES_G2" not in os.environ
    zkmi.init(0)
    T.TABLE_SHAPES[20] = (1 << 19, 1 << 19)
    info = T.table_case("bn128", group, 20, "alternate_coarse")
    print("case", "bn128", group, 20, "alternate_coarse", json.dumps(dict(info, lanes_per_sum=zkmi.lib().zkmi_msm_rowcol_lanes(group))), flush=True)
    print("lanes ok")


def run_child(call, env):
    code = "import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_msm_rowcol_lanes as t\nt.%s\n" % (ROOT, os.path.join(ROOT, "tests"), call)
    base = {k: v for k, v in os.environ.items() if k not in ("ZKMI_RC_LANES", "ZKMI_RC_LANES_G2")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(base, **env))
    assert r.returncode == 0 and "lanes ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    print(r.stdout)
    return {tuple(f[1:5]): json.loads(l.split(None, 5)[5].rsplit("}", 1)[0] + "}") for l in r.stdout.splitlines() for f in [l.split()] if f[:1] == ["case"]}


@pytest.mark.parametrize("lps", H.LANES)
@pytest.mark.parametrize("name,group", T.PAIRS)
def test_forced_lanes(name, group, lps):
    got = run_child("child_lanes(%r, %d, %d)" % (name, group, lps), {"ZKMI_RC_LANES": str(lps), "ZKMI_RC_LANES_G2": str(lps)})
    assert sorted(got) == sorted((name, str(group), str(c), kind) for c in (13, 14, 15) for kind in KINDS + (LEVELS if c == 13 else ()))
    for (_, _, c, _), info in got.items():
        rbits, cbits = P.grid_bits(int(c))
        assert (info["rbits"], info["cbits"], info["r29_buckets"]) == (rbits, cbits, 1), info


def test_refused_unless_8_16_32_64():
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_msm_rowcol_lanes as t\nfrom snarkjs_amd import zkmi\nzkmi.init(0)\n"
            "terms, Wd = t.terms_of('constant', 13, t.M.order('bn128'), 64)\nzkmi.lib().zkmi_msm_set_window_bits(13)\n"
            "try:\n    t.T.run_case('bn128', 1, terms, 13, Wd, 4)\nexcept zkmi.ZkmiError as e:\n    print('refused', e)\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, ZKMI_RC_LANES="24"))
    assert r.returncode == 0 and "refused" in r.stdout and "8, 16, 32 or 64" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize("group", (1, 2))
def test_default_pick_at_c20(group):
    got = run_child("child_c20(%d)" % group, {"ZKMI_TABLE_C": "20"})
    (info,) = got.values()
    assert (info["c"], info["rbits"], info["cbits"], info["rowcol_kernel"], info["bitsums"]) == (20, 9, 10, T.WAVE29_G2 if group == 2 else T.WAVE29, 1), info
    # the defaults of csrc/msm_select.hpp as tests/test_msm_rowcol_lanes_host.py pins them through the pick itself
    assert info["lanes_per_sum"] == (H.G2_LANES if group == 2 else H.G1_LANES), info
