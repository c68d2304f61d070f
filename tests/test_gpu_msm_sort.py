"""The front half of every MSM — csrc/msm_sort.hip: msm_sort, the signed-digit recoding and digit sort (csrc/msm.cuh: k_msm_count / _scatter, k_rsort_*) and
the lane schedule (k_msm_classify / k_msm_assign) — looked at directly through zkmi_msm_sort_probe_dev (include/zkmi_diag.h), which runs the product's own
msm_sort and hands back what it built and which of its sorts it took. The work is integer work, so everything is compared exactly with the numpy
restatement of tests/msm_sort_ref.py (checked on the CPU by tests/test_msm_sort_ref_host.py): the bucket counts, their prefix sums, the multiset of
entries of every bucket, the lane totals, the lane groups, their order, the giants table and the number of chunks. The cases (msm_sort_ref.CASES) are the
smallest shapes on each side of every rule by which msm_sort picks a path, and each must report the path written next to it: a case that stops reaching
its branch fails.

The four switches ZKMI_RSORT, ZKMI_RSORT_FUSED, ZKMI_RSORT_STAGED and ZKMI_RSORT_LB are read once per process: each setting runs the whole list in a
process of its own, and the same content checks are applied to what it prints."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import msm_patterns as P
import msm_sort_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_content(cs, info, a):
    """assertions 1 - 7 and 9 of a case: everything the sort and the schedule built, against the reference; the path itself is the caller's to judge"""
    ref = R.case_reference(cs)
    total, counts_ref = ref["total"], ref["counts"]
    assert (info["c"], info["Wd"], info["W"], info["nb"], info["total"], info["nw"]) == (cs.c, cs.Wd, cs.W, 1 << (cs.c - 1), total, cs.nw), info
    cap = R.lane_cap(cs.n, cs.c, cs.Wd, bool(cs.table))
    assert info["cap"] == cap, info
    counts = a["counts"].astype(np.int64)
    # 1. counts = bincount of the reference keys
    assert len(counts) == total and np.array_equal(counts, counts_ref), np.nonzero(counts != counts_ref)[0][:8]
    # 2. starts = exclusive prefix sum of counts: the lists of all buckets form one flat array
    excl = np.concatenate([[0], np.cumsum(counts_ref)[:-1]])
    assert np.array_equal(a["starts"].astype(np.int64), excl), np.nonzero(a["starts"] != excl)[0][:8]
    # 3. bucket by bucket the reference's multiset of entries
    assert info["entries"] == len(ref["keys"]) == len(a["sorted"])
    bucket = np.repeat(np.arange(total, dtype=np.int64), counts_ref)
    got = a["sorted"][np.lexsort((a["sorted"], bucket))]
    assert np.array_equal(bucket, ref["keys"]) and np.array_equal(got, ref["ents"]), np.nonzero(got != ref["ents"])[0][:8]
    # 4. meta[0..2] = all lanes, lanes of multi-lane groups, giants
    j = R.lanes_log(counts_ref, cap)
    m = R.schedule_totals(counts_ref, cap)
    print(cs.name, "info", info, "meta", a["meta"].tolist(), "reference", m)
    assert tuple(int(x) for x in a["meta"]) == m and (info["lanes"], info["giants"]) == (m[0], m[2])
    # 5. every non-empty bucket owns lanes(cnt) consecutive lanes that begin at a multiple of that number and carry lane_sub = 0 .. L-1
    lane_g, lane_sub = a["lane_g"].astype(np.int64), a["lane_sub"].astype(np.int64)
    assert len(lane_g) == len(lane_sub) == m[0] and lane_g.max(initial=0) < total
    first = np.nonzero(np.concatenate([[True], lane_g[1:] != lane_g[:-1]]))[0] if m[0] else np.zeros(0, np.int64)
    run_g, run_len = lane_g[first], np.diff(np.concatenate([first, [m[0]]]))
    assert len(np.unique(run_g)) == len(run_g), "a bucket's lanes are not contiguous"
    assert np.array_equal(np.sort(run_g), np.nonzero(counts_ref)[0])
    assert np.array_equal(run_len, 1 << j[run_g]) and not (first % run_len).any()
    assert np.array_equal(lane_sub, np.arange(m[0]) - np.repeat(first, run_len))
    # 6. keys never increase along the lanes
    keys = R.keys_of(counts_ref, cap)[lane_g]
    assert (keys[1:] <= keys[:-1]).all()
    # 7. the giants table, as a set
    lane0 = np.zeros(total, np.int64)
    lane0[run_g] = first
    want = {(int(g), int(lane0[g]) >> R.MSM_LOG_TB, 1 << (int(j[g]) - R.MSM_LOG_TB)) for g in np.nonzero(j > R.MSM_LOG_TB)[0]}
    rows = [tuple(int(x) for x in a["giants"][3 * k:3 * k + 3]) for k in range(m[2])]
    assert len(a["giants"]) == 3 * m[2] and len(set(rows)) == len(rows) and set(rows) == want
    # 9. chunks = sum ceil(size / 8192) over the partitions above fused_cap (all of them when it is 0), sizes by the reference
    if info["radix"]:
        assert info["parts"] == total >> info["lb"]
        assert info["chunks"] == R.chunk_count(R.partition_sizes(ref["keys"], total, info["lb"]), info["fused_cap"]), info
    else:
        assert (info["lb"], info["parts"], info["fused_cap"], info["staged"], info["chunks"]) == (0, 0, 0, 0, 0), info


def reported_path(info):
    return {k: info[k] for k in ("radix", "lb", "parts", "fused_cap", "staged")}


@pytest.fixture(scope="module")
def device():
    from snarkjs_amd import zkmi
    zkmi.init()
    return zkmi.lib()


@pytest.mark.parametrize("cs", R.CASES, ids=repr)
def test_sort_and_schedule(device, cs):
    """every case in this process (no switch set): content, and the literal path of the case table (assertion 8)"""
    info, a = R.run_probe(cs)
    check_content(cs, info, a)
    assert reported_path(info) == cs.path, (cs, info)
    if cs.chunks is not None:
        assert info["chunks"] == cs.chunks, (cs, info)


def test_probe_entry_checks(device):
    """the probe validates like zkmi_msm_dev and refuses arrays that are too small instead of writing past them"""
    import ctypes as C
    from snarkjs_amd import zkmi
    L, cs = device, R.CASE["a-ones"]
    d_s = zkmi.DeviceBuffer.from_host(R.case_input(cs)[0])
    info = zkmi.MsmSortInfo()
    none = (None, None, 0, None, 0, None, None, 0, None, 0, None)
    assert L.zkmi_msm_sort_probe_dev(None, cs.n, 32, 15, 0, None, *none, C.byref(info)) != 0
    assert L.zkmi_msm_sort_probe_dev(d_s.ptr, cs.n, 32, 15, 0, None, *none, None) != 0
    assert L.zkmi_msm_sort_probe_dev(d_s.ptr, 0, 32, 15, 0, None, *none, C.byref(info)) != 0
    assert L.zkmi_msm_sort_probe_dev(d_s.ptr, cs.n, 65, 15, 0, None, *none, C.byref(info)) != 0
    assert L.zkmi_msm_sort_probe_dev(d_s.ptr, cs.n, 32, 21, 0, None, *none, C.byref(info)) != 0
    assert L.zkmi_msm_sort_probe_dev(d_s.ptr, cs.n, 32, 15, cs.n - 1, None, *none, C.byref(info)) != 0
    zkmi.check(L.zkmi_msm_sort_probe_dev(d_s.ptr, cs.n, 32, 15, 0, None, *none, C.byref(info)))
    assert (info.total, info.entries, info.lanes, info.giants) == (1 << 14, cs.n, 512, 1)
    counts = np.full(info.total, 0xAAAAAAAA, np.uint32)
    assert L.zkmi_msm_sort_probe_dev(d_s.ptr, cs.n, 32, 15, 0, None, zkmi.ptr(counts), None, info.total - 1, None, 0, None, None, 0, None, 0, None, C.byref(info)) != 0
    assert b"too small" in L.zkmi_last_error() and (counts == 0xAAAAAAAA).all()
    d_s.free()


# ---- the switches -------------------------------------------------------------------------------------------------------------------------------------
SWITCHES = {"counting-sort": {"ZKMI_RSORT": "0"}, "chunked-level-2": {"ZKMI_RSORT_FUSED": "0"}, "direct-level-1": {"ZKMI_RSORT_STAGED": "0"},
            "512-bucket-partitions": {"ZKMI_RSORT_LB": "9"}}


_switch_runs = {}


def switch_run(setting):
    """what one child process (one GPU process, started when the first case of its setting asks, and never a second time: a child that failed fails every
    case of its setting with what it left) printed for every case: {case name: (info, arrays)}"""
    if setting not in _switch_runs:
        import tempfile
        with tempfile.TemporaryDirectory(prefix="zkmi_sort_") as tmp:
            code = "import sys; sys.path[:0] = [%r, %r]\nimport msm_sort_ref as R\nR.child_main(%r)\n" % (ROOT, os.path.join(ROOT, "tests"), tmp)
            r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, **SWITCHES[setting]))
            out = {}
            if r.returncode == 0 and "sort cases done" in r.stdout:
                for f in (l.split() for l in r.stdout.splitlines()):
                    if f[:1] == ["sort"] and len(f) == 5:
                        with np.load(f[4]) as z:
                            a = {k: z[k] for k in R.ARRAYS}
                        out[f[1]] = (json.loads(f[2]), a, f[3])
            _switch_runs[setting] = out if sorted(out) == sorted(R.CASE) else "exit status %d\n" % r.returncode + r.stdout[-2000:] + r.stderr[-3000:]
    assert isinstance(_switch_runs[setting], dict), _switch_runs[setting]
    return _switch_runs[setting]


@pytest.mark.parametrize("cs", R.CASES, ids=repr)
@pytest.mark.parametrize("setting", SWITCHES)
def test_sort_and_schedule_under_switch(setting, cs):
    """the same list with one switch of csrc/msm_sort.hip set: the content checks unchanged, and the path the switch asks for"""
    info, a, sha = switch_run(setting)[cs.name]
    assert R.digest(a) == sha
    check_content(cs, info, a)
    if setting == "counting-sort":
        assert info["radix"] == 0, info
        return
    assert info["radix"] == cs.path["radix"], info                                       # none of the other three moves the choice between the two sorts
    if not info["radix"]:
        return
    if setting == "chunked-level-2":
        assert info["lb"] == 11 and info["fused_cap"] == 0 and info["staged"] == R.path_rules(cs.c, cs.Wd, cs.W, cs.n, fused_on=False)["staged"], info
    elif setting == "direct-level-1":
        assert info["staged"] == 0 and (info["lb"], info["fused_cap"]) == (cs.path["lb"], cs.path["fused_cap"]), info
    else:
        p9 = (cs.W << (cs.c - 1)) >> 9
        if cs.Wd * cs.n // p9 <= 13500 and cs.c > 9:
            assert (info["lb"], info["fused_cap"], info["parts"]) == (9, 15000, p9), info
        else:
            assert cs.name not in ("b-uniform", "b-edges", "b-skew", "b-ones", "h") and (info["lb"], info["fused_cap"]) == (11, 0), info


# ---- end to end: 4-byte scalars on the main table width -------------------------------------------------------------------------------------------------
N_TABLE = 1 << 16


def child_table_c20():
    """runs in a process with ZKMI_TABLE_C=20: a table over 2^16 geometric bases (BN254 G1) and one MSM of 4-byte scalars over it — the NW = 1 radix sort with
    the direct level-1 scatter (case i), through zkmi_msm_table_dev"""
    import ctypes as C
    from snarkjs_amd import zkmi
    assert os.environ["ZKMI_TABLE_C"] == "20"
    zkmi.init(0)
    L, cs = zkmi.lib(), R.CASE["i"]
    d_b = zkmi.DeviceBuffer(N_TABLE * 64)
    zkmi.check(L.zkmi_gen_geometric_bases_dev(0, 1, N_TABLE, 7, 11, d_b.ptr))
    h = C.c_uint64(0)
    zkmi.check(L.zkmi_msm_table_build(0, 1, d_b.ptr, N_TABLE, C.byref(h)))
    d_s = zkmi.DeviceBuffer.from_host(R.case_input(cs)[0])
    out = np.zeros(96, np.uint8)
    zkmi.check(L.zkmi_msm_table_dev(h, d_s.ptr, N_TABLE, 4, zkmi.ptr(out)))
    print("msm", out.tobytes().hex())
    info, _ = R.run_probe(cs)                                  # the sort that MSM began with took the path of case i
    print("path", json.dumps(info))
    zkmi.check(L.zkmi_msm_table_release(h))
    print("table ok")


def test_table_msm_c20_four_byte_scalars():
    """zkmi_msm_table_dev with 4-byte scalars over a c = 20 table of 2^16 bases against the closed form sum s_i 7 11^i mod r (no MSM in the reference)"""
    cs = R.CASE["i"]
    assert (cs.n, cs.sb) == (N_TABLE, 4)
    code = "import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_msm_sort as t\nt.child_table_c20()\n" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, ZKMI_TABLE_C="20"))
    assert r.returncode == 0 and "table ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    lines = dict(l.split(None, 1) for l in r.stdout.splitlines() if l.split()[:1] in (["msm"], ["path"]))
    order = int(json.load(open(os.path.join(ROOT, "tests", "golden", "bn128_kernel_vectors.json")))["r"])
    k = P.closed_form(R.case_input(cs)[0], 4, P.discrete_logs("geometric", N_TABLE, order), order)
    assert k != 0
    got = np.frombuffer(bytes.fromhex(lines["msm"].strip()), np.uint8)
    assert np.array_equal(O.to_affine(0, 1, got), O.to_affine(0, 1, O.generator_mul(0, 1, k)))
    info = json.loads(lines["path"])
    assert reported_path(info) == cs.path and info["nw"] == 1, info
