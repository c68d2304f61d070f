"""The resident-table MSM (csrc/msm29.cuh, msm_sort.hip, msm_host.hpp: msm_reduce) at every window width msm_precomp_c can pick, on both curves and
both groups, against closed forms: the bases are k_i * G for known k_i, so every result is (sum s_i k_i mod r) * G, computed in Python integers and
one scalar multiplication of the CPU oracle. No MSM is involved in the reference. The scalars come from tests/msm_patterns.py: they hit the edges of the
signed-digit recoding and of the bucket grid on purpose (tests/test_msm_patterns_host.py shows that they do). Affine bytes are compared exactly.

ZKMI_TABLE_C=<c> (csrc/zkmi_api.hip: table_build) fixes the width of every table a process builds, whatever their size; it is read once, so each
width runs in a process of its own."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import msm_patterns as P
import oracle_lib as O
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [("bn128", 1), ("bn128", 2), ("bls12381", 1), ("bls12381", 2)]
SMALL, LARGE = 3077, 1 << 14          # below the radix sort's threshold at every width (33 * 3077 < 2^17), and above it for every c >= 12


@functools.lru_cache(None)
def order(name):
    return int(json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"{name}_kernel_vectors.json")))["r"])


@functools.lru_cache(None)
def logs(kind, n, name):
    return P.discrete_logs(kind, n, order(name))


@functools.lru_cache(None)
def scalar_set(kind, c, n, sb=32):
    """one array per (kind, width, size), shared by every case and every curve / group; never written to"""
    if kind == "uniform":
        a = P.scalars("uniform", 0, n, sb, seed=P.UNIFORM_SEED + n + sb)
    elif kind == "witness":
        a = synth.witness_like(P.UNIFORM_SEED + n, n)
    else:
        a = P.edge_set(c, n, sb) if kind == "digit_edges" else P.skew_set(c, n)
    a.setflags(write=False)
    return a


def affine_of(name, group, k):
    c = O.CURVE_ID[name]
    return O.to_affine(c, group, O.generator_mul(c, group, k))


def expect(name, group, sc, sb, base_kind, n, k):
    return affine_of(name, group, P.closed_form(sc, sb, logs(base_kind, n, name), order(name), k))


def make_bases(name, group, kind, n):
    """k_i * G on the device: the geometric ones by their own generator, any others from their discrete logarithms"""
    from snarkjs_amd import zkmi
    c, L = O.CURVE_ID[name], zkmi.lib()
    d_b = zkmi.DeviceBuffer(n * 2 * group * O.n8q(c))
    if kind == "geometric":
        zkmi.check(L.zkmi_gen_geometric_bases_dev(c, group, n, 7, 11, d_b.ptr))
    else:
        d_k = zkmi.DeviceBuffer.from_host(P.logs_bytes(logs(kind, n, name)))
        zkmi.check(L.zkmi_gen_bases_from_scalars_dev(c, group, d_k.ptr, n, d_b.ptr))
        d_k.free()
    return d_b


def build_table(name, group, d_b, n):
    from snarkjs_amd import zkmi
    L, h = zkmi.lib(), C.c_uint64(0)
    zkmi.check(L.zkmi_msm_table_build(O.CURVE_ID[name], group, d_b.ptr, n, C.byref(h)))
    cv, g, m = C.c_int(-1), C.c_int(-1), C.c_size_t(0)
    zkmi.check(L.zkmi_msm_table_info(h, C.byref(cv), C.byref(g), C.byref(m)))
    assert (cv.value, g.value, m.value) == (O.CURVE_ID[name], group, n)
    return h


# ---- every width ---------------------------------------------------------------------------------------------------------------------------
def width_cases():
    """(resident bases, kind of bases, kind of scalars, scalar bytes, terms of the MSM)"""
    for n, bases in ((SMALL, "special"), (LARGE, "geometric")):
        for kind in ("uniform", "digit_edges", "skew"):
            yield n, bases, kind, 32, n
        yield n, bases, "uniform", 32, n - 5
        yield n, bases, "uniform", 32, 1
        if n == SMALL:                                    # the byte-wise branch of load_scalar, and fewer digits than the table has rows
            for sb in (4, 31, 1):
                yield n, bases, "digit_edges", sb, n


def child_every_width(c):
    """runs in the process started by test_table_msm_every_width: one hex line per result"""
    from snarkjs_amd import zkmi
    assert int(os.environ["ZKMI_TABLE_C"]) == c
    zkmi.init(0)
    L = zkmi.lib()
    for name, group in PAIRS:
        q8 = O.n8q(O.CURVE_ID[name])
        for n, bases in ((SMALL, "special"), (LARGE, "geometric")):
            d_b = make_bases(name, group, bases, n)
            if bases == "special":
                print("pts", name, group, d_b.to_host(64 * 2 * group * q8).tobytes().hex())
            h = build_table(name, group, d_b, n)
            for i, (n_, _, kind, sb, k) in enumerate(width_cases()):
                if n_ != n:
                    continue
                d_s = zkmi.DeviceBuffer.from_host(scalar_set(kind, c, n, sb))
                out = np.zeros(3 * group * q8, np.uint8)
                counted = (n, kind) == (LARGE, "skew")        # the device's own count of the mixed additions of this MSM (zkmi_msm_stats)
                zkmi.check(L.zkmi_msm_stats(int(counted)))
                zkmi.check(L.zkmi_msm_table_dev(h, d_s.ptr, k, sb, zkmi.ptr(out)))
                print("msm", name, group, i, out.tobytes().hex())
                if counted:
                    print("adds", name, group, int(L.zkmi_msm_accum_additions(0)))
                d_s.free()
            zkmi.check(L.zkmi_msm_table_release(h))
            d_b.free()
    print("widths ok")


@pytest.mark.parametrize("c", P.WIDTHS)
def test_table_msm_every_width(c):
    """Window tables of width c over 3077 bases with doubled, negated and infinite points among them and over 2^14 geometric ones, on both curves and
    groups: uniform scalars (all, a prefix, one term), the digit-edge set at 32, 31, 4 and 1 bytes, and the skewed set that fills giant buckets."""
    code = "import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_msm_widths as t\nt.child_every_width(%d)\n" % (ROOT, os.path.join(ROOT, "tests"), c)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, ZKMI_TABLE_C=str(c)))
    assert r.returncode == 0 and "widths ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l.split() for l in r.stdout.splitlines()]
    cases = list(width_cases())
    got = {(f[1], int(f[2]), int(f[3])): np.frombuffer(bytes.fromhex(f[4]), np.uint8) for f in lines if f[:1] == ["msm"]}
    assert sorted(got) == sorted((name, group, i) for name, group in PAIRS for i in range(len(cases)))
    pts = {(f[1], int(f[2])): np.frombuffer(bytes.fromhex(f[3]), np.uint8) for f in lines if f[:1] == ["pts"]}
    assert sorted(pts) == sorted(PAIRS)
    # The table really has width c: the accumulation performs one mixed addition per non-zero digit (no geometric base is the point at infinity), and
    # the number of non-zero digits of the skewed set is different at each of the ten widths
    values = P.ints(scalar_set("skew", c, LARGE), 32)
    digits = sum(len(P.signed_digits(v, c, 32)[0]) * values.count(v) for v in set(values))
    adds = {(f[1], int(f[2])): int(f[3]) for f in lines if f[:1] == ["adds"]}
    assert adds == {pair: digits for pair in PAIRS}, (c, digits, adds)
    bad = []
    for name, group in PAIRS:
        want = np.concatenate([affine_of(name, group, k) for k in logs("special", SMALL, name)[:64]])      # the base generator is not trusted blindly
        assert np.array_equal(pts[name, group], want), (name, group, "generated bases")
        for i, (n, bases, kind, sb, k) in enumerate(cases):
            sc = scalar_set(kind, c, n, sb)
            if not np.array_equal(O.to_affine(O.CURVE_ID[name], group, got[name, group, i]), expect(name, group, sc, sb, bases, n, k)):
                bad.append((name, group, n, kind, sb, k))
    assert not bad, (c, bad)


# ---- batched calls at the default width ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from snarkjs_amd import zkmi
    zkmi.init(0)
    return zkmi.lib()


N_MULTI = (1 << 13) + 6               # PLONK's SRS slice for a domain of 2^13; msm_precomp_c gives c = 13: 64 rows x 64 columns, the smallest wave shape
# (kind of scalars, terms) of the MSMs of each call: kinds are mixed within a call, so that the jobs of one reduction batch differ in their empty buckets
MULTI_CALLS = [[("digit_edges", N_MULTI)],
               [("skew", N_MULTI), ("uniform", 77)],
               [("uniform", N_MULTI - 5), ("digit_edges", 0), ("witness", 1)],
               [("uniform", N_MULTI), ("digit_edges", N_MULTI - 5), ("skew", 0), ("witness", 77)]]
ENQUEUED_CALL = [("witness", N_MULTI), ("skew", N_MULTI), ("digit_edges", 77), ("uniform", 1)]


@pytest.mark.parametrize("name,group", PAIRS)
def test_table_msm_multi_vs_closed_form(lib, name, group):
    """zkmi_msm_table_multi_dev with 1 to 4 MSMs per call (msm_reduce with njobs 1 to 4), its enqueue / collect halves on pipeline slot 1 and the
    variant that converts from Montgomery form inside the call: every output against its own closed form, an MSM of no terms is all-zero bytes."""
    from snarkjs_amd import zkmi
    L, cid, n, c, r = lib, O.CURVE_ID[name], N_MULTI, 13, order(name)
    pj = 3 * group * O.n8q(cid)
    d_b = make_bases(name, group, "special", n)
    h = build_table(name, group, d_b, n)
    dev = {kind: zkmi.DeviceBuffer.from_host(scalar_set(kind, c, n)) for kind in ("uniform", "digit_edges", "skew", "witness")}

    def check_outputs(call, out, what):
        for i, (kind, k) in enumerate(call):
            jac = out[i * pj:(i + 1) * pj]
            if k == 0:
                assert not jac.any(), (what, i)
            else:
                assert np.array_equal(O.to_affine(cid, group, jac), expect(name, group, scalar_set(kind, c, n), 32, "special", n, k)), (what, i, kind, k)

    def arrays(call, bufs):
        return (C.c_void_p * len(call))(*[bufs[kind].ptr for kind, _ in call]), (C.c_size_t * len(call))(*[k for _, k in call])
    try:
        for call in MULTI_CALLS:
            p, ks = arrays(call, dev)
            out = np.full(len(call) * pj, 0xA5, np.uint8)
            zkmi.check(L.zkmi_msm_table_multi_dev(h, p, ks, len(call), 32, zkmi.ptr(out)))
            check_outputs(call, out, "multi")
        p, ks = arrays(ENQUEUED_CALL, dev)
        out = np.full(4 * pj, 0xA5, np.uint8)
        try:
            zkmi.check(L.zkmi_pipeline_select(1))
            zkmi.check(L.zkmi_msm_table_multi_enqueue_dev(h, p, ks, 4, 32))
            zkmi.check(L.zkmi_msm_table_multi_collect(h, 4, zkmi.ptr(out)))
        finally:
            L.zkmi_pipeline_select(0)
        check_outputs(ENQUEUED_CALL, out, "enqueue / collect on slot 1")
        # Montgomery input: s_i * 2^256 mod r for s_i < r, with 0, 1 and r - 1 among them; the library does not refuse G2, so G2 is held to the same closed form
        plain, mont = {}, {}
        for kind in ("uniform", "digit_edges"):
            s = [v % r for v in P.ints(scalar_set(kind, c, n), 32)]
            s[:3] = [0, 1, r - 1]
            plain[kind] = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in s), np.uint8)
            mont[kind] = zkmi.DeviceBuffer.from_host(np.frombuffer(b"".join(((v << 256) % r).to_bytes(32, "little") for v in s), np.uint8))
        call = [("uniform", n), ("digit_edges", n - 5), ("uniform", 3)]
        p, ks = arrays(call, mont)
        out = np.full(3 * pj, 0xA5, np.uint8)
        zkmi.check(L.zkmi_msm_table_multi_enqueue_mont_dev(h, p, ks, 3))
        zkmi.check(L.zkmi_msm_table_multi_collect(h, 3, zkmi.ptr(out)))
        for i, (kind, k) in enumerate(call):
            want = affine_of(name, group, P.closed_form(plain[kind], 32, logs("special", n, name), r, k))
            assert np.array_equal(O.to_affine(cid, group, out[i * pj:(i + 1) * pj]), want), ("from Montgomery", i, kind, k)
        for b in mont.values():
            b.free()
    finally:
        zkmi.check(L.zkmi_msm_table_release(h))
        for b in dev.values():
            b.free()
        d_b.free()


# ---- the caller-owned path -----------------------------------------------------------------------------------------------------------------
# the widths of test_gpu_parity.py: test_msm_window_sweep. Without a table every digit has a bucket set of its own (W = Wd): widths above 16 would
# need gigabytes of Fq2 buckets at this size and are left out
SWEEP_WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 16)
N_SWEEP = 3000


@pytest.mark.parametrize("name,group", [("bn128", 2), ("bls12381", 1), ("bls12381", 2)])
def test_msm_dev_window_sweep_all_groups(lib, name, group):
    """zkmi_msm_dev (W = Wd bucket sets, k_msm_wsum in place of the bit sums) at every width zkmi_msm_set_window_bits takes in the BN254 G1 sweep, on the
    three other curve / group pairs: the digit-edge set of each width over bases with doubled, negated and infinite points; 48-byte scalars at one width."""
    from snarkjs_amd import zkmi
    L, cid, n = lib, O.CURVE_ID[name], N_SWEEP
    d_b = make_bases(name, group, "special", n)
    out = np.zeros(3 * group * O.n8q(cid), np.uint8)
    try:
        for c in SWEEP_WIDTHS:
            zkmi.check(L.zkmi_msm_set_window_bits(c))
            for kind, sb in (("digit_edges", 32),) + ((("uniform", 48),) if c == 12 else ()):
                sc = scalar_set(kind, c, n, sb)
                d_s = zkmi.DeviceBuffer.from_host(sc)
                zkmi.check(L.zkmi_msm_dev(cid, group, d_b.ptr, d_s.ptr, n, sb, zkmi.ptr(out)))
                d_s.free()
                assert np.array_equal(O.to_affine(cid, group, out), expect(name, group, sc, sb, "special", n, n)), (c, kind, sb)
    finally:
        L.zkmi_msm_set_window_bits(0)
        d_b.free()
