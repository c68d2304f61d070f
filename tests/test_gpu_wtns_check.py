"""wtns.check on the device: zkmi_r1cs_load / zkmi_r1cs_check / zkmi_r1cs_check_dev (csrc/r1cs_check.hip) against the Python restatement of the reference's loop
(tests/wtns_check_vectors.py) — constraint counts around the slice edges, row lengths around the segment and the cut-row edges in A, in B and in C, repeated
signals and wide values, batches, witnesses in device memory, every refusal with a resident key kept intact —, the drivers of snarkjs_amd/wtns_check.py on every
golden case, and one heavy-tailed circuit of 2^12 constraints."""
import ctypes as C

import numpy as np
import pytest

import wtns_check_vectors as V
from snarkjs_amd import wtns_check, zkmi
from snarkjs_amd.workloads import synth_r1cs as S
from test_wtns_check_host import CASES, IDS, hold_driver_to_golden

pytestmark = pytest.mark.gpu
CURVES = ["bn128", "bls12381"]
COUNTS = [0, 1, 2, 21, 22, 43, 300]            # 3 n rows = segments: 63 | 66 and 129 cross the slice edges 64 and 128
LENGTHS = [0, 1, 31, 32, 33, 64, 65, 2049]     # 2049 terms: 65 partial sums, the fold's stride loop runs twice
NONE = V.NONE
GUARD = 8
_key = [0x7e57000000000000]
_cache = {}


def new_key():
    _key[0] += 1
    return _key[0]


def section2(cons):
    return V.read_r1cs(S.write_r1cs("bn128", 1, 0, 0, cons))["constraints"]


def wbytes(wit):
    return b"".join(int(v).to_bytes(32, "little") for v in wit)


def spoil(curve, wit, *signals):
    w = list(wit)
    for s in signals:
        w[s] = (w[s] + 1) % S.R[curve]
    return w


def expected(curve, cons_bytes, n_c, wits):
    out = []
    for w in wits:
        bad = V.first_bad(cons_bytes, n_c, V.R[curve], wbytes(w))
        out.append(NONE if bad is None else bad)
    return out


def load(curve, cons_bytes, n_c, n_vars, key=None, pages=None):
    zkmi.init()
    key = key or new_key()
    pg = zkmi.pages_of(pages if pages is not None else cons_bytes)
    return zkmi.lib().zkmi_r1cs_load(zkmi.CURVE_ID[curve], pg.pages, n_c, n_vars, key), key


def run(key, wits, n_vars, dev=False):
    """first_bad of a batch, written between guard words"""
    n = len(wits)
    data = np.frombuffer(b"".join(wbytes(w) for w in wits), np.uint8)
    out = np.full(GUARD + n + GUARD, 0xA5A5A5A5, np.uint32)
    p_out = C.c_void_p(out.ctypes.data + 4 * GUARD)
    if dev:
        buf = zkmi.DeviceBuffer.from_host(data)
        try:
            zkmi.check(zkmi.lib().zkmi_r1cs_check_dev(key, C.c_void_p(buf.ptr), data.size, n, p_out))
        finally:
            buf.free()
    else:
        zkmi.check(zkmi.lib().zkmi_r1cs_check(key, zkmi.ptr(data), data.size, n, p_out))
    assert (out[:GUARD] == 0xA5A5A5A5).all() and (out[GUARD + n:] == 0xA5A5A5A5).all(), "first_bad written outside its n words"
    return [int(v) for v in out[GUARD:GUARD + n]]


def solved(cons, i):
    return max(s for s, _ in cons[i][2])


def counted(curve, n):
    """n satisfied constraints, a good witness, and witnesses failing at the first, a middle and the last constraint that solves a signal"""
    if (curve, n) not in _cache:
        nv, _, _, cons, wit = S.satisfiable_circuit(curve, n, seed=0xc0 + n)
        wits = [wit]
        for i in sorted({0, 3 * (n // 6), 3 * ((n - 1) // 3)}) if n else []:
            wits.append(spoil(curve, wit, solved(cons, i)))
        sec = section2(cons)
        _cache[(curve, n)] = (nv, sec, wits, expected(curve, sec, n, wits))
    return _cache[(curve, n)]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("curve", CURVES)
def test_constraint_counts_around_the_slice_edges(curve, n):
    nv, sec, wits, want = counted(curve, n)
    assert want[0] == NONE and (n == 0 or (want[1] == 0 and len(set(want)) == len(want)))
    rc, key = load(curve, sec, n, nv)
    zkmi.check(rc)
    try:
        assert run(key, wits, nv) == want
        assert run(key, wits[::-1], nv, dev=True) == want[::-1]
        assert run(key, wits[:1], nv) == want[:1]
    finally:
        zkmi.lib().zkmi_r1cs_release(key)


def rows_circuit(curve):
    """24 + 3 constraints: every length of LENGTHS once in A, once in B, once in C. The LAST term of each 2049-term row is moved onto a signal of its own (same
    value), so that a bad value there touches that row alone, in its last segment (the one of a single term)."""
    if ("rows", curve) not in _cache:
        rows = {(3 * j + m, m): L for j, L in enumerate(LENGTHS) for m in range(3)}             # constraint 3 j + m: length L in matrix m
        nv, _, _, cons, wit = S.satisfiable_circuit(curve, 27, seed=0x10f, rows=rows)
        cons, wit = [tuple(list(lc) for lc in c) for c in cons], list(wit)
        own = {}
        for (i, m), L in rows.items():
            assert len(cons[i][m]) == L, (i, m, L, len(cons[i][m]))
            if L == 2049:
                s, c = cons[i][m][-1]
                cons[i][m][-1] = (len(wit), c)
                own[m] = (i, len(wit))
                wit.append(wit[s])
        sec = section2(cons)
        assert V.first_bad(sec, 27, V.R[curve], wbytes(wit)) is None
        _cache[("rows", curve)] = (len(wit), sec, wit, own, cons)
    return _cache[("rows", curve)]


@pytest.mark.parametrize("curve", CURVES)
def test_row_lengths_in_a_b_and_c_and_the_fold_of_cut_rows(curve):
    nv, sec, wit, own, cons = rows_circuit(curve)
    assert set(own) == {0, 1, 2}
    wits = [wit] + [spoil(curve, wit, own[m][1]) for m in range(3)] + [spoil(curve, wit, cons[5][0][0][0])]
    want = expected(curve, sec, 27, wits)
    assert want[0] == NONE and [want[1 + m] for m in range(3)] == [own[m][0] for m in range(3)], "the bad value in the last segment of a 2049-term row fails that constraint alone"
    rc, key = load(curve, sec, 27, nv)
    zkmi.check(rc)
    try:
        assert run(key, wits, nv) == want
        assert run(key, wits, nv, dev=True) == want
        # the constraint section in pages that end inside a count and inside a record
        rc, k2 = load(curve, sec, 27, nv, pages=[sec[:2], sec[2:4 + 17], sec[4 + 17:1000], b"", sec[1000:]])
        zkmi.check(rc)
        assert run(k2, wits, nv) == want
        zkmi.lib().zkmi_r1cs_release(k2)
    finally:
        zkmi.lib().zkmi_r1cs_release(key)


@pytest.mark.parametrize("curve", CURVES)
def test_repeated_signals_wide_values_and_a_batch_cut_into_passes(curve):
    r = S.R[curve]
    nv, _, _, cons, wit = S.satisfiable_circuit(curve, 45, seed=0xdd, dups=True, wide=True, rows={(4, 0): 70, (7, 1): 40, (9, 2): 66})
    desc = [tuple(sorted(lc, key=lambda t: -t[0]) for lc in c) for c in S.satisfiable_circuit(curve, 45, seed=0xdd, wide=True, rows={(4, 0): 70})[3]]
    sec, sec_desc = section2(cons), section2(desc)
    assert any(len(lc) != len({s for s, _ in lc}) for c in cons for lc in c) and any(v >= r for v in wit)
    # a batch of 5: witnesses 1 and 3 fail at different constraints, the others hold
    wits = [wit, spoil(curve, wit, solved(cons, 30)), [v + r if v + r < 1 << 256 else v for v in wit], spoil(curve, wit, solved(cons, 12), solved(cons, 42)), wit]
    want = expected(curve, sec, 45, wits)
    assert want == [NONE, 30, NONE, 12, NONE]
    rc, key = load(curve, sec, 45, nv)
    zkmi.check(rc)
    try:
        assert run(key, wits, nv) == want
        assert run(key, wits, nv, dev=True) == want
        per = 32 * nv + 96 * 45
        try:
            zkmi.check(zkmi.lib().zkmi_diag_set_r1cs_budget(3 * per))                     # two witnesses a pass, or so: the batch is cut
            assert run(key, wits, nv) == want
            zkmi.check(zkmi.lib().zkmi_diag_set_r1cs_budget(1))                           # one witness a pass
            assert run(key, wits, nv, dev=True) == want
        finally:
            zkmi.check(zkmi.lib().zkmi_diag_set_r1cs_budget(0))
    finally:
        zkmi.lib().zkmi_r1cs_release(key)
    w2 = S.satisfiable_circuit(curve, 45, seed=0xdd, wide=True, rows={(4, 0): 70})[4]
    rc, key = load(curve, sec_desc, 45, len(w2))
    zkmi.check(rc)
    try:
        bad = spoil(curve, w2, max(s for s, _ in desc[21][2]))
        assert run(key, [w2, bad], len(w2)) == expected(curve, sec_desc, 45, [w2, bad]) == [NONE, 21]
    finally:
        zkmi.lib().zkmi_r1cs_release(key)


def test_every_refusal_leaves_a_resident_key_intact():
    nv, sec, wits, want = counted("bn128", 22)
    L = zkmi.lib()
    rc, key = load("bn128", sec, 22, nv)
    zkmi.check(rc)
    out = np.zeros(4, np.uint32)
    w = np.frombuffer(wbytes(wits[0]), np.uint8)

    def refused(rc, code=2):
        assert rc == code, (rc, L.zkmi_last_error())
        assert run(key, wits, nv) == want, "the resident key still answers"
    try:
        pg = zkmi.pages_of(sec)
        refused(L.zkmi_r1cs_load(2, pg.pages, 22, nv, new_key()))                                            # an unknown curve
        refused(L.zkmi_r1cs_load(-1, pg.pages, 22, nv, new_key()))
        refused(L.zkmi_r1cs_load(0, pg.pages, 22, nv, 0))                                                    # key 0
        null = zkmi.Pages(None, None, 1)
        refused(L.zkmi_r1cs_load(0, null, 22, nv, new_key()))                                                # null pointers
        ptrs, lens = (C.c_void_p * 1)(None), (C.c_size_t * 1)(len(sec))
        refused(L.zkmi_r1cs_load(0, zkmi.Pages(C.cast(ptrs, C.POINTER(C.c_void_p)), C.cast(lens, C.POINTER(C.c_size_t)), 1), 22, nv, new_key()))
        refused(L.zkmi_r1cs_load(0, pg.pages, (1 << 31) // 3 + 1, nv, new_key()), 4)                         # 3 n >= 2^31
        refused(L.zkmi_r1cs_load(0, pg.pages, 23, nv, new_key()))                                            # the section ends early
        refused(load("bn128", sec[:-10], 22, nv)[0])
        refused(load("bn128", sec, 22, nv - 1)[0])                                                          # a signal id >= nVars (the last solved signal)
        refused(L.zkmi_r1cs_load(0, pg.pages, 22, nv + 1, key))                                              # the resident key described differently
        refused(L.zkmi_r1cs_load(1, pg.pages, 22, nv, key))
        refused(L.zkmi_r1cs_load(0, pg.pages, 21, nv, key))
        refused(L.zkmi_r1cs_load(0, pg.pages, 22, nv, key), 0)                                               # ... and as it is: nothing to do
        refused(L.zkmi_r1cs_check(0, zkmi.ptr(w), w.size, 1, zkmi.ptr(out)))                                 # key 0
        refused(L.zkmi_r1cs_check(new_key(), zkmi.ptr(w), w.size, 1, zkmi.ptr(out)))                         # nothing resident under the key
        refused(L.zkmi_r1cs_check(key, None, w.size, 1, zkmi.ptr(out)))
        refused(L.zkmi_r1cs_check(key, zkmi.ptr(w), w.size, 1, None))
        refused(L.zkmi_r1cs_check(key, zkmi.ptr(w), w.size - 32, 1, zkmi.ptr(out)))                          # witness_len
        refused(L.zkmi_r1cs_check(key, zkmi.ptr(w), w.size, 2, zkmi.ptr(out)))
        refused(L.zkmi_r1cs_check_dev(key, None, w.size, 1, zkmi.ptr(out)))
        refused(L.zkmi_r1cs_check_dev(0, None, w.size, 1, zkmi.ptr(out)))
        refused(L.zkmi_r1cs_check(key, zkmi.ptr(w), 0, 0, zkmi.ptr(out)), 0)                                 # no witnesses: nothing to do
        assert (out == 0).all()
    finally:
        L.zkmi_r1cs_release(key)
    assert L.zkmi_r1cs_check(key, zkmi.ptr(w), w.size, 1, zkmi.ptr(out)) == 2, "released"
    assert L.zkmi_r1cs_release(key) == 0


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_drivers_on_the_golden_cases(c):
    hold_driver_to_golden(c, wtns_check.Device)


def test_checker_keeps_the_layout_resident():
    by = {c["name"]: c for c in CASES}
    for curve in CURVES:
        with wtns_check.Checker(V.golden_file(by[f"{curve}_good"]["r1cs"])) as ck:
            ws = [V.golden_file(by[f"{curve}_{n}"]["wtns"]) for n in ("good", "bad_two", "bad_last", "wide_witness", "bad_first")]
            assert ck.check_many(ws) == [None, 9, 12, None, 0]
            assert ck.check(ws[0]) is True and ck.check(ws[2]) is False
            raw = b"".join(V.read_wtns(w)["witness"] for w in ws[:3])
            buf = zkmi.DeviceBuffer.from_host(np.frombuffer(raw, np.uint8))
            try:
                assert ck.check_dev(buf.ptr, 3) == [None, 9, 12]
            finally:
                buf.free()


def test_heavy_tailed_circuit_of_4096_constraints():
    nv, _, _, cons, wit = S.satisfiable_circuit("bn128", 4096, seed=0x7a11, tail=True)
    assert max(len(c[0]) for c in cons) > 500 and sum(len(c[0]) <= 3 for c in cons) > 3000
    sec = section2(cons)
    wits = [wit, spoil("bn128", wit, solved(cons, 4095)), spoil("bn128", wit, solved(cons, 2049), solved(cons, 3000)), spoil("bn128", wit, 700)]
    want = expected("bn128", sec, 4096, wits)
    assert want[:3] == [NONE, 4095, 2049] and want[3] != NONE
    rc, key = load("bn128", sec, 4096, nv)
    zkmi.check(rc)
    try:
        assert run(key, wits, nv) == want
    finally:
        zkmi.lib().zkmi_r1cs_release(key)
