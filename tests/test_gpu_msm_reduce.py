"""The back half of every MSM — the lane-partial folds behind the bucket accumulation (csrc/msm.cuh: k_msm_tree, k_msm_giant), the row / column sums
(k_msm_rowcol_wave29, _wave29_g2, _wave, k_msm_rowcol + k_msm_fold) and the weighted sums (k_msm_bitsums, _bitsums_lds, k_msm_wsum) — looked at stage by
stage through zkmi_msm_stage_probe_dev (include/zkmi_diag.h), which runs the product's own entry point and hands back the finished buckets, the row /
column sums, the result and the kernels the picks chose. The inputs of tests/msm_reduce_patterns.py place a chosen point in a chosen bucket, so that the
additions of these stages meet equal, opposite and infinite operands (tests/test_msm_reduce_patterns_host.py counts that they do); everything expected
is arithmetic mod r on discrete logarithms and one scalar multiplication of the CPU oracle per distinct value. Every comparison is exact.

The switches that change a kernel of these stages are read once per process: each setting runs its cases in a process of its own.

Which case runs which kernel, and the rare branches the model counts for it there (every case asserts the kernel from the info record):
  k_msm_rowcol_wave29        G1, tables of c = 13, 15 (both curves), 17, 20 (BN254) and caller-owned bases at c = 13, 15; its Compact instantiation: BLS12-381 under
                             ZKMI_COMPACT_CODE=31. dbl_xyzz29 behind padd29_ld: constant (every tree level; the shares from two buckets per lane on), alternate_fine
                             (shares, c >= 15); the cancellation: the alternate patterns; the inf_s skip: those, one_per_row, cancelled; the
                             cn[g] && !xyzz29_words_inf gate: cancelled, and the fat buckets of opposite copies
  k_msm_rowcol_wave29_g2     G2, the same cases: dbl29_lds behind padd29_lds, the cancellation, the skip and the gate by the same patterns
  k_msm_rowcol_wave          every pair under ZKMI_R29_REDUCE=0 ZKMI_R29_REDUCE_G2=0 and BLS12-381 G2 under ZKMI_COMPACT_CODE=31, c = 13, 15: G1 the doubling and the
                             cancellation of pt_add_inl, G2 pt_dbl_lds behind pt_add_lds and the inf_s skip of lds_tree_sum
  k_msm_rowcol + k_msm_fold  every pair at c = 12, and at c = 13, 15 under ZKMI_ROWCOL_WAVE=0: doubling and cancellation of pt_add_inl (G1) and pt_add (G2) in the
                             shares (an even stride apart: equal signs) and in the folds
  k_msm_bitsums, _bitsums_lds  every table case and the 4-byte caller-owned one (W = 3); G2 runs _lds, and k_msm_bitsums under ZKMI_ROWCOL_WAVE=0: constant doubles
                             (all row sums equal), alternate_rows cancels, the other alternate patterns feed it infinity alone
  k_msm_wsum                 caller-owned bases with 32-byte scalars, 20 and 18 bucket sets: constant doubles in the suffix scan, alternate_rows cancels
  k_msm_tree, k_msm_giant    the fat buckets (c = 16, cap 8: 8 lanes, and 256 lanes = two tree blocks): with equal copies all 7 + 254 + 1 additions are doublings
Left unreached: the cancellation of pt_add inside k_msm_tree / k_msm_giant (a lane's share depends on the order of the bucket's list, which the sort does not
fix: with negated copies the bucket is infinity in any order, the branches on the way are not pinned); the second level of k_msm_wsum with its pt_dbl
scaling (rows of more than one block: c >= 18 without a table); merge mode and the auxiliary-stream reduction of a proof."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import msm_patterns as P
import msm_reduce_patterns as M
import msm_sort_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [("bn128", 1), ("bn128", 2), ("bls12381", 1), ("bls12381", 2)]
# csrc/msm_select.hpp: MsmAccumKernel and MsmRowcolKernel as the info record reports them
ACCUM29, ACCUM29_COMPACT, ACCUM29_G2S, ACCUM29_G2, ACCUM29_G2_COMPACT = 0, 2, 4, 5, 6
WAVE29, WAVE29_COMPACT, WAVE29_G2, WAVE, STAGED = 0, 1, 2, 3, 4
INFO = ("c", "W", "nb", "rbits", "cbits", "accum_kernel", "rowcol_kernel", "r29_buckets", "bitsums", "cap", "lanes", "multi_lanes", "giants")


@functools.lru_cache(None)
def affine_of(name, group, k):
    cid = O.CURVE_ID[name]
    return O.to_affine(cid, group, O.generator_mul(cid, group, k)).tobytes()


def points_of(name, group, values):
    """the affine points values[i] * G as one array of bytes; 0 is the point at infinity, all-zero"""
    pb = 2 * group * O.n8q(O.CURVE_ID[name])
    uniq = sorted(set(values))
    table = np.stack([np.frombuffer(affine_of(name, group, v) if v else bytes(pb), np.uint8) for v in uniq])
    pos = {v: i for i, v in enumerate(uniq)}
    return table[np.fromiter((pos[v] for v in values), np.int64, len(values))].reshape(-1)


def expected_kernels(name, group, c, env=None):
    """csrc/msm_select.hpp: msm_accum_pick / msm_rowcol_pick for R'-form bases (a window table, or the library's copy of caller-owned bases), with the
    switches of this process or of the child's environment: (accum kernel, rowcol kernel, R'-form buckets)"""
    from snarkjs_amd import zkmi
    env = os.environ if env is None else env
    on = lambda k: not (k in env and int(env[k]) == 0)
    limbs, wave_c = (14 if name == "bls12381" else 9), (c - 1) // 2 >= 6
    cc = zkmi.lib().zkmi_compact_code()
    wave = on("ZKMI_ROWCOL_WAVE") and wave_c
    if group == 2:
        r29 = wave and on("ZKMI_R29_REDUCE_G2") and not cc & 8
        if on("ZKMI_G2_SPLIT") and not (limbs == 14 and not on("ZKMI_G2_SPLIT_BLS")):
            acc = ACCUM29_G2S
        else:
            acc = ACCUM29_G2_COMPACT if limbs == 14 and cc & 2 else ACCUM29_G2
        return acc, (WAVE29_G2 if r29 else WAVE) if wave else STAGED, int(r29)
    r29 = wave and on("ZKMI_R29_REDUCE")
    acc = ACCUM29_COMPACT if limbs == 14 and cc & 1 else ACCUM29
    return acc, ((WAVE29_COMPACT if limbs == 14 and cc & 4 else WAVE29) if r29 else WAVE) if wave else STAGED, int(r29)


def probe(L, h, cid, group, d_b, d_s, n, sb):
    """zkmi_msm_stage_probe_dev: a first call without arrays for the sizes, a second one that fetches them -> (info dict, buckets, rowcol, result)"""
    from snarkjs_amd import zkmi
    info, pb = zkmi.MsmStageInfo(), 2 * group * O.n8q(cid)
    args = (h, cid, group, d_b, d_s, n, sb)
    zkmi.check(L.zkmi_msm_stage_probe_dev(*args, None, 0, None, 0, None, C.byref(info)))
    nbk, nrc = info.W * info.nb, (2 * info.W) << info.cbits
    buckets, rowcol, result = np.full(nbk * pb, 0xA5, np.uint8), np.full(nrc * pb, 0xA5, np.uint8), np.full(3 * pb // 2, 0xA5, np.uint8)
    first = {k: getattr(info, k) for k in INFO}
    zkmi.check(L.zkmi_msm_stage_probe_dev(*args, zkmi.ptr(buckets), nbk, zkmi.ptr(rowcol), nrc, zkmi.ptr(result), C.byref(info)))
    assert first == {k: getattr(info, k) for k in INFO}
    return first, buckets, rowcol, result


def run_case(name, group, terms, c, W, sb, resident=0, n_terms=None, env=None):
    """One MSM over the bases and scalars of `terms` through the probe and through the ordinary entry point: a window table over `resident` bases (the
    width c is what the table must have picked) or, with resident = 0, caller-owned bases at the width the caller has set. Compares buckets, row / column
    sums and result with the model, exactly, and returns the info record."""
    from snarkjs_amd import zkmi
    L, cid, r = zkmi.lib(), O.CURVE_ID[name], M.order(name)
    pb = 2 * group * O.n8q(cid)
    n = len(terms) if n_terms is None else n_terms
    logs = [v for _, _, v in terms] + [1] * (max(resident, n) - len(terms))
    sc = np.concatenate([M.scalars_of(terms, c, sb), np.zeros((n - len(terms)) * sb, np.uint8)])
    d_k = zkmi.DeviceBuffer.from_host(P.logs_bytes(logs))
    d_b = zkmi.DeviceBuffer(len(logs) * pb)
    d_s = zkmi.DeviceBuffer.from_host(sc)
    h = C.c_uint64(0)
    try:
        zkmi.check(L.zkmi_gen_bases_from_scalars_dev(cid, group, d_k.ptr, len(logs), d_b.ptr))
        if resident:
            zkmi.check(L.zkmi_msm_table_build(cid, group, d_b.ptr, resident, C.byref(h)))
        info, buckets, rowcol, result = probe(L, h.value, cid, group, d_b.ptr, d_s.ptr, n, sb)
        out = np.full(3 * pb // 2, 0xA5, np.uint8)
        if resident:
            zkmi.check(L.zkmi_msm_table_dev(h, d_s.ptr, n, sb, zkmi.ptr(out)))
        else:
            zkmi.check(L.zkmi_msm_dev(cid, group, d_b.ptr, d_s.ptr, n, sb, zkmi.ptr(out)))
    finally:
        if h.value:
            L.zkmi_msm_table_release(h)
        for b in (d_k, d_b, d_s):
            b.free()
    rbits, cbits = P.grid_bits(c)
    assert (info["c"], info["W"], info["nb"], info["rbits"], info["cbits"]) == (c, W, 1 << (c - 1), rbits, cbits), info
    V, counts, rows, cols, k = M.expected(terms, c, W, r)
    want = points_of(name, group, V)
    bad = np.nonzero((buckets.reshape(-1, pb) != want.reshape(-1, pb)).any(axis=1))[0]
    assert not len(bad), ("buckets", name, group, c, len(bad), bad[:8].tolist(), [counts[b] for b in bad[:8]], info)
    want = points_of(name, group, M.rowcol_layout(rows, cols, c))
    bad = np.nonzero((rowcol.reshape(-1, pb) != want.reshape(-1, pb)).any(axis=1))[0]
    assert not len(bad), ("row / column sums", name, group, c, len(bad), bad[:8].tolist(), info)
    for what, jac in (("result", result), ("entry point", out)):
        if k == 0:
            assert not jac.any(), (what, name, group, c, info)
        else:
            assert np.array_equal(O.to_affine(cid, group, jac), np.frombuffer(affine_of(name, group, k), np.uint8)), (what, name, group, c, info)
    acc, rck, r29 = expected_kernels(name, group, c, env)
    assert (info["accum_kernel"], info["rowcol_kernel"], info["r29_buckets"]) == (acc, rck, r29), (name, group, c, info)
    return info


@pytest.fixture(scope="module")
def lib():
    from snarkjs_amd import zkmi
    zkmi.init(0)
    return zkmi.lib()


# ---- window tables at the widths a table picks for its size ------------------------------------------------------------------------------------------
# (c, resident bases, terms): 12 the staged sums; 13 the smallest wave form, one bucket per lane; 15 two per lane; 17 four per lane
TABLE_SHAPES = {12: (4096, 2048), 13: (8192, 4096), 15: (1 << 14, 1 << 14), 17: (1 << 17, 1 << 16)}


def table_case(name, group, c, kind, env=None):
    resident, k = TABLE_SHAPES[c]
    terms = M.pattern(kind, c, M.order(name), max(k, min(resident, 2 << (c - 1))) if kind == "cancelled" else k)
    info = run_case(name, group, terms, c, 1, 32, resident=resident, env=env)
    assert info["bitsums"] == 1, info                                   # one bucket set: plain bit sums and a Horner on the host
    return info


@pytest.mark.parametrize("kind", M.PATTERNS)
@pytest.mark.parametrize("c", (12, 13, 15))
@pytest.mark.parametrize("name,group", PAIRS)
def test_table_stages(lib, name, group, c, kind):
    info = table_case(name, group, c, kind)
    assert (info["rowcol_kernel"] == STAGED) == (c == 12), info


@pytest.mark.parametrize("kind", M.PATTERNS)
@pytest.mark.parametrize("group", (1, 2))
def test_table_stages_c17(lib, group, kind):
    """four buckets per lane of the wave sums (BN254)"""
    table_case("bn128", group, 17, kind)


# ---- lists spread over several lanes: k_msm_tree and k_msm_giant ------------------------------------------------------------------------------------------
N_FAT = 1 << 16


@pytest.mark.parametrize("same_sign", (True, False), ids=("equal", "opposite"))
@pytest.mark.parametrize("name,group", PAIRS)
def test_fat_buckets(lib, name, group, same_sign):
    """2^3 cap and 256 cap copies of one point in a bucket each, at 2^16 terms (the rest are zero scalars): every lane partial is the same point and every
    level of k_msm_tree and of k_msm_giant's tree is a doubling; with every second copy negated the bucket sums to infinity whichever way the sort
    ordered its list, and the row / column sums meet a bucket that has entries and no point"""
    c = 16
    cap = R.lane_cap(N_FAT, c, P.digits_of(32, c), True)
    info = run_case(name, group, M.fat(c, M.order(name), cap, same_sign), c, 1, 32, resident=N_FAT, n_terms=N_FAT)
    assert (info["cap"], info["multi_lanes"], info["giants"], info["lanes"]) == (cap, 8 + 256, 1, 8 + 256 + 2), info


# ---- caller-owned bases: one bucket set per window ----------------------------------------------------------------------------------------------------
def dev_case(lib, name, group, c, kind, sb):
    """the pattern in window 0, in a middle window and in the top one as far as that holds scalar bits"""
    r, Wd, nb = M.order(name), P.digits_of(sb, c), 1 << (c - 1)
    terms = []
    for i, w in enumerate(sorted({0, Wd // 2, Wd - 1})):
        top_bits = 8 * sb - c * w
        if top_bits <= 0:
            continue
        terms += M.pattern(kind, c, r, nb, window=w, limit=None if top_bits >= c else (1 << top_bits) - 1, seed=i)
    try:
        assert lib.zkmi_msm_set_window_bits(c) == 0
        return run_case(name, group, terms, c, Wd, sb)
    finally:
        lib.zkmi_msm_set_window_bits(0)


@pytest.mark.parametrize("kind", M.PATTERNS)
@pytest.mark.parametrize("c", (13, 15))
@pytest.mark.parametrize("name,group", PAIRS)
def test_dev_stages_many_windows(lib, name, group, c, kind):
    """32-byte scalars: 20 and 18 bucket sets, too many arrays for the bit sums: k_msm_wsum"""
    info = dev_case(lib, name, group, c, kind, 32)
    assert info["bitsums"] == 0 and info["rowcol_kernel"] != STAGED, info


@pytest.mark.parametrize("kind", M.PATTERNS)
@pytest.mark.parametrize("name,group", PAIRS)
def test_dev_stages_four_byte_scalars(lib, name, group, kind):
    """three bucket sets: the bit sums with W > 1"""
    info = dev_case(lib, name, group, 13, kind, 4)
    assert info["bitsums"] == 1 and info["W"] == 3, info


# ---- jobs of different character in one row / column launch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,group", PAIRS)
def test_table_multi_four_patterns(lib, name, group):
    """zkmi_msm_table_multi_dev over one table of G and -G, 4096 of each (c = 13): the four scalar vectors pick, bucket by bucket, G (constant), G or -G by
    the parity of row + column (alternate_fine), by the parity of the row (alternate_rows), or both (every bucket cancels). Checked by the
    result, since the probe looks at one job."""
    from snarkjs_amd import zkmi
    cid, r, c = O.CURVE_ID[name], M.order(name), 13
    nb, pj = 1 << (c - 1), 3 * group * O.n8q(cid)
    _, cbits = P.grid_bits(c)
    row, col = np.arange(nb) >> cbits, np.arange(nb) & ((1 << cbits) - 1)
    minus = {"constant": np.zeros(nb, bool), "alternate_fine": (row + col) & 1 == 1, "alternate_rows": row & 1 == 1}
    jobs, want = [], []
    for kind in ("constant", "alternate_fine", "alternate_rows", "cancelled"):
        s = np.zeros((2 * nb, 8), np.uint32)
        if kind == "cancelled":
            s[:nb, 0] = s[nb:, 0] = np.arange(nb) + 1
            want.append(0)
        else:
            s[:nb, 0] = np.where(minus[kind], 0, np.arange(nb) + 1)
            s[nb:, 0] = np.where(minus[kind], np.arange(nb) + 1, 0)
            want.append(sum((b + 1) * (-1 if m else 1) for b, m in enumerate(minus[kind].tolist())) % r)
        jobs.append(zkmi.DeviceBuffer.from_host(s.view(np.uint8).reshape(-1)))
    d_k = zkmi.DeviceBuffer.from_host(P.logs_bytes([1] * nb + [r - 1] * nb))
    d_b = zkmi.DeviceBuffer(2 * nb * 2 * group * O.n8q(cid))
    h = C.c_uint64(0)
    try:
        zkmi.check(lib.zkmi_gen_bases_from_scalars_dev(cid, group, d_k.ptr, 2 * nb, d_b.ptr))
        zkmi.check(lib.zkmi_msm_table_build(cid, group, d_b.ptr, 2 * nb, C.byref(h)))
        out = np.full(4 * pj, 0xA5, np.uint8)
        zkmi.check(lib.zkmi_msm_table_multi_dev(h, (C.c_void_p * 4)(*[b.ptr for b in jobs]), (C.c_size_t * 4)(*[2 * nb] * 4), 4, 32, zkmi.ptr(out)))
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
            assert np.array_equal(O.to_affine(cid, group, jac), np.frombuffer(affine_of(name, group, k), np.uint8)), i


def test_probe_entry_checks(lib):
    """the probe validates like the entry points and refuses arrays that are too small instead of writing past them"""
    from snarkjs_amd import zkmi
    cid, c = 0, 12
    terms = M.pattern("generic", c, M.order("bn128"), 2048)
    d_k = zkmi.DeviceBuffer.from_host(M.logs_of(terms))
    d_b = zkmi.DeviceBuffer(len(terms) * 64)
    d_s = zkmi.DeviceBuffer.from_host(M.scalars_of(terms, c, 32))
    info = zkmi.MsmStageInfo()
    try:
        zkmi.check(lib.zkmi_gen_bases_from_scalars_dev(cid, 1, d_k.ptr, len(terms), d_b.ptr))
        assert lib.zkmi_msm_set_window_bits(c) == 0
        none = (None, 0, None, 0, None)
        assert lib.zkmi_msm_stage_probe_dev(0, cid, 1, d_b.ptr, None, len(terms), 32, *none, C.byref(info)) != 0
        assert lib.zkmi_msm_stage_probe_dev(0, cid, 1, None, d_s.ptr, len(terms), 32, *none, C.byref(info)) != 0
        assert lib.zkmi_msm_stage_probe_dev(0, cid, 1, d_b.ptr, d_s.ptr, 0, 32, *none, C.byref(info)) != 0
        assert lib.zkmi_msm_stage_probe_dev(0, cid, 1, d_b.ptr, d_s.ptr, len(terms), 32, *none, None) != 0
        assert lib.zkmi_msm_stage_probe_dev(12345, cid, 1, d_b.ptr, d_s.ptr, len(terms), 32, *none, C.byref(info)) != 0
        zkmi.check(lib.zkmi_msm_stage_probe_dev(0, cid, 1, d_b.ptr, d_s.ptr, len(terms), 32, *none, C.byref(info)))
        assert (info.c, info.W, info.nb, info.rowcol_kernel, info.bitsums) == (c, 22, 2048, STAGED, 0)
        buckets = np.full(22 * 2048 * 64, 0xAA, np.uint8)
        assert lib.zkmi_msm_stage_probe_dev(0, cid, 1, d_b.ptr, d_s.ptr, len(terms), 32, zkmi.ptr(buckets), 22 * 2048 - 1, None, 0, None, C.byref(info)) != 0
        assert b"too small" in lib.zkmi_last_error() and (buckets == 0xAA).all() and info.nb == 2048
        try:                                                    # refused while the pipeline slot holds work, like the entry points
            zkmi.check(lib.zkmi_pipeline_select(1))
            h = C.c_uint64(0)
            zkmi.check(lib.zkmi_msm_table_build(cid, 1, d_b.ptr, len(terms), C.byref(h)))
            zkmi.check(lib.zkmi_msm_table_multi_enqueue_dev(h, (C.c_void_p * 1)(d_s.ptr), (C.c_size_t * 1)(len(terms)), 1, 32))
            assert lib.zkmi_msm_stage_probe_dev(0, cid, 1, d_b.ptr, d_s.ptr, len(terms), 32, *none, C.byref(info)) != 0
            out = np.zeros(96, np.uint8)
            zkmi.check(lib.zkmi_msm_table_multi_collect(h, 1, zkmi.ptr(out)))
            zkmi.check(lib.zkmi_msm_table_release(h))
        finally:
            lib.zkmi_pipeline_select(0)
    finally:
        lib.zkmi_msm_set_window_bits(0)
        for b in (d_k, d_b, d_s):
            b.free()


# ---- the switches, and the widest table: a process each ----------------------------------------------------------------------------------------------------
SWITCHES = {"staged-sums": ({"ZKMI_ROWCOL_WAVE": "0"}, PAIRS),
            "generic-wave-sums": ({"ZKMI_R29_REDUCE": "0", "ZKMI_R29_REDUCE_G2": "0"}, PAIRS),
            "g2-parked-in-lds": ({"ZKMI_G2_SPLIT": "0"}, [("bn128", 2), ("bls12381", 2)]),
            "called-products": ({"ZKMI_COMPACT_CODE": "31"}, [("bls12381", 1), ("bls12381", 2)])}


def child_switch(setting):
    from snarkjs_amd import zkmi
    zkmi.init(0)
    env, pairs = SWITCHES[setting]
    assert all(os.environ.get(k) == v for k, v in env.items())
    for name, group in pairs:
        for c in (13, 15):
            for kind in M.PATTERNS:
                print("case", name, group, c, kind, json.dumps(table_case(name, group, c, kind)), flush=True)
    print("stages ok")


def child_c20():
    """BN254 G1, a c = 20 table over 2^19 bases: 512 rows of 1024 columns, sixteen and eight buckets per lane"""
    from snarkjs_amd import zkmi
    assert os.environ["ZKMI_TABLE_C"] == "20"
    zkmi.init(0)
    TABLE_SHAPES[20] = (1 << 19, 1 << 19)
    for kind in M.PATTERNS:
        print("case", "bn128", 1, 20, kind, json.dumps(table_case("bn128", 1, 20, kind)), flush=True)
    print("stages ok")


def run_child(call, env):
    code = "import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_msm_reduce as t\nt.%s\n" % (ROOT, os.path.join(ROOT, "tests"), call)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0 and "stages ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    return {tuple(f[1:5]): json.loads(l.split(None, 5)[5]) for l in r.stdout.splitlines() for f in [l.split()] if f[:1] == ["case"]}


@pytest.mark.parametrize("setting", SWITCHES)
def test_table_stages_under_switch(setting):
    """the c = 13 and c = 15 cases with one setting that changes a kernel of these stages: the same exact comparisons inside the child (run_case, which
    also holds the info record to the kernels the setting asks for), and here that every case ran and took the kernel the setting is there for"""
    env, pairs = SWITCHES[setting]
    got = run_child("child_switch(%r)" % setting, env)
    assert sorted(got) == sorted((name, str(group), str(c), kind) for name, group in pairs for c in (13, 15) for kind in M.PATTERNS)
    for (name, group, c, kind), info in got.items():
        if setting == "staged-sums":
            assert (info["rowcol_kernel"], info["r29_buckets"]) == (STAGED, 0), info
        elif setting == "generic-wave-sums":
            assert (info["rowcol_kernel"], info["r29_buckets"]) == (WAVE, 0), info
        elif setting == "g2-parked-in-lds":
            assert info["accum_kernel"] in (ACCUM29_G2, ACCUM29_G2_COMPACT), info
        elif group == "1":
            assert (info["accum_kernel"], info["rowcol_kernel"]) == (ACCUM29_COMPACT, WAVE29_COMPACT), info
        else:
            assert (info["rowcol_kernel"], info["r29_buckets"]) == (WAVE, 0), info      # bit 3: the Fq2 sums go back to the generic kernel


def test_table_stages_c20():
    got = run_child("child_c20()", {"ZKMI_TABLE_C": "20"})
    assert sorted(got) == sorted(("bn128", "1", "20", kind) for kind in M.PATTERNS)
    assert all((i["c"], i["rbits"], i["cbits"], i["rowcol_kernel"], i["bitsums"]) == (20, 9, 10, WAVE29, 1) for i in got.values()), got
