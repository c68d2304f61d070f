"""The aggregated PLONK / FFLONK check on the device (VerifyingKey.verify_all / verify_all_raw / verify_many_fast) against the per-proof
verifier of the same key and against tests/aggregate_verify_vectors.py: verify_all == all(code == 1 for code in verify_codes) on batches of
distinct device proofs with and without one tampered member and with each structural failure, the trace sums against the Python restatement,
reproducibility under a seed, verify_many_fast == verify_many, and the isolation rules of the per-proof verifiers."""
import os
import random

import numpy as np
import pytest

import aggregate_verify_vectors as AV
import fflonk_verify_vectors as FV
import plonk_verify_vectors as PV

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 4096, 4097)
CASES = [("plonk", "plonk_bn128_small"), ("plonk", "plonk_bls12381_small"), ("fflonk", "fflonk_bn128_small")]


class Case:
    """one protocol and key: the resident key, 4 097 distinct device proofs of the golden witness (fresh blinding each), the tampers"""

    def __init__(self, proto, tag):
        from snarkjs_amd import plonk, fflonk, plonk_verify, fflonk_verify
        self.proto, self.tag = proto, tag
        self.vec = PV if proto == "plonk" else FV
        self.mod = plonk_verify if proto == "plonk" else fflonk_verify
        self.vk, self.pubs, self.golden = self.vec.golden(tag + ".json")
        self.R = self.mod._FQ[self.vk.get("curve", "bn128")][3]
        zkey = open(os.path.join(self.vec.GOLDEN, tag + ".zkey"), "rb").read()
        wtns = open(os.path.join(self.vec.GOLDEN, tag + ".wtns"), "rb").read()
        res = (plonk if proto == "plonk" else fflonk).prove_many(zkey, [wtns] * max(SIZES))
        assert res[0]["publicSignals"] == self.pubs
        self.proofs = [r["proof"] for r in res]
        last = (lambda p: p["Wxiw"][0]) if proto == "plonk" else (lambda p: p["polynomials"]["W2"][0])
        assert len({last(p) for p in self.proofs}) == max(SIZES)
        self.key = self.mod.VerifyingKey(self.vk)

    def bad_eval(self, p):
        if self.proto == "plonk":
            return PV.with_(p, eval_a=str((int(p["eval_a"]) + 1) % self.R))
        return FV.with_eval(p, "z", (int(p["evaluations"]["z"]) + 1) % self.R)

    def off_curve(self, p):
        if self.proto == "plonk":
            bad = list(p["A"])
            bad[0] = str((int(bad[0]) + 1) % self.key.p)
            return PV.with_(p, A=bad)
        return FV.with_point(p, "C1", FV.off_curve(p["polynomials"]["C1"]))


_cases = {}


@pytest.fixture(params=CASES, ids=lambda c: c[1])
def case(request):
    if request.param not in _cases:
        _cases[request.param] = Case(*request.param)
    return _cases[request.param]


def agree(c, lists, proofs, seed):
    """verify_all, verify_many_fast and the per-proof verifier on one batch; returns the per-proof codes"""
    codes = c.key.verify_codes(lists, proofs)
    assert c.key.verify_all(lists, proofs, seed) == all(x == 1 for x in codes)
    assert c.key.verify_many_fast(lists, proofs, seed) == c.key.verify_many(lists, proofs) == [x == 1 for x in codes]
    return codes


@pytest.mark.parametrize("n", SIZES)
def test_equivalence(case, n):
    c = case
    rnd = random.Random("eq %s %d" % (c.tag, n))
    seed = AV.seed_of("eq %s %d" % (c.tag, n))
    proofs, lists = c.proofs[:n], [c.pubs] * n
    assert agree(c, lists, proofs, seed) == [1] * n
    assert c.key.verify_all(lists, proofs) is True                               # a seed from the OS
    at = rnd.randrange(n)
    tampered = proofs[:at] + [c.bad_eval(proofs[at])] + proofs[at + 1:]
    assert agree(c, lists, tampered, seed) == [0 if i == at else 1 for i in range(n)]
    # each structural failure: a commitment off the curve (-2), a public signal out of range (-1, caught while packing)
    at = rnd.randrange(n)
    off = proofs[:at] + [c.off_curve(proofs[at])] + proofs[at + 1:]
    assert agree(c, lists, off, seed) == [-2 if i == at else 1 for i in range(n)]
    recs, pb, n_sig, _ = c.key.pack(lists, off)
    ok, codes = c.key.verify_all_raw(recs, pb, n_sig, n, seed)
    assert not ok and [int(x) for x in codes] == [-2 if i == at else 1 for i in range(n)]
    if c.pubs:
        big = lists[:at] + [[str(c.R)] + list(c.pubs[1:])] + lists[at + 1:]
        assert agree(c, big, proofs, seed) == [-1 if i == at else 1 for i in range(n)]
        # the same on the device: r itself has a 32-byte form
        recs, pb, n_sig, _ = c.key.pack(lists, proofs)
        pb = pb.copy()
        pb[32 * len(c.pubs) * at:32 * len(c.pubs) * at + 32] = np.frombuffer(int(c.R).to_bytes(32, "little"), np.uint8)
        ok, codes = c.key.verify_all_raw(recs, pb, n_sig, n, seed)
        assert not ok and [int(x) for x in codes] == [-1 if i == at else 1 for i in range(n)]


def test_wrong_signal_count_and_empty_batch(case):
    from snarkjs_amd import zkmi
    c = case
    more = [list(c.pubs) + ["1"]] * 3
    assert agree(c, more, c.proofs[:3], AV.seed_of("count")) == [-3] * 3
    recs, pb, n_sig, _ = c.key.pack(more, c.proofs[:3])
    with pytest.raises(zkmi.ZkmiError, match=c.mod.MESSAGES[-3]):
        c.key.verify_all_raw(recs, pb, n_sig, 3, AV.seed_of("count"))
    assert c.key.verify_all([], []) is True and c.key.verify_many_fast([], []) == []
    ok, codes = c.key.verify_all_raw(np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    assert ok and codes.size == 0


def test_trace_and_reproducibility(case):
    c = case
    n = 65
    proofs, lists = c.proofs[100:100 + n], [c.pubs] * n
    s1, s2 = AV.seed_of("trace 1 " + c.tag), AV.seed_of("trace 2 " + c.tag)
    ok, codes, sp, sq = c.key.aggregate_trace(lists, proofs, s1)
    want = AV.restate(c.proto, c.vk, list(zip(lists, proofs)), s1)
    assert (ok, [int(x) for x in codes], sp, sq) == want and ok and sp is not None and sq is not None
    assert c.key.aggregate_trace(lists, proofs, s1)[2:] == (sp, sq)
    ok2, _, sp2, sq2 = c.key.aggregate_trace(lists, proofs, s2)
    assert ok2 and sp2 != sp and sq2 != sq
    # a tampered member and a structural failure: the sums of the restatement, ok false under both seeds
    bad = proofs[:7] + [c.bad_eval(proofs[7])] + proofs[8:40] + [c.off_curve(proofs[40])] + proofs[41:]
    got = c.key.aggregate_trace(lists, bad, s1)
    want = AV.restate(c.proto, c.vk, list(zip(lists, bad)), s1)
    assert (got[0], [int(x) for x in got[1]], got[2], got[3]) == want and not got[0]
    assert not c.key.aggregate_trace(lists, bad, s2)[0]


def test_timers_report_the_aggregated_kernels(case):
    from snarkjs_amd import zkmi
    c = case
    L = zkmi.lib()
    assert c.key.verify_all([c.pubs] * 130, c.proofs[:130], AV.seed_of("ms"))
    ms = (zkmi.C.c_double * 3)()
    zkmi.check(getattr(L, "zkmi_%s_aggregate_phase_ms" % c.proto)(ms))
    total = getattr(L, "zkmi_%s_verify_last_ms" % c.proto)()
    assert all(x > 0 for x in ms) and total >= sum(ms) * 0.99
    c.key.verify_codes([c.pubs], c.proofs[:1])
    zkmi.check(getattr(L, "zkmi_%s_aggregate_phase_ms" % c.proto)(ms))
    assert list(ms) == [-1.0] * 3


def test_isolation(case):
    """a Groth16 proof submitted to each pipeline slot BEFORE a 4 097-proof aggregated batch and finished AFTER it keeps its bytes, and the three
    per-proof verifiers give the same verdicts before and after an aggregated batch"""
    import oracle_lib as OL
    import verify_vectors as GV
    from snarkjs_amd import groth16, binfile, zkmi, groth16_verify as gv, plonk_verify as pv, fflonk_verify as fv
    c = case
    gd = PV.GOLDEN
    L = zkmi.lib()
    n = 4097
    lists, proofs = [c.pubs] * n, c.proofs[:n]
    recs, pb, n_sig, _ = c.key.pack(lists, proofs)
    seed = AV.seed_of("iso " + c.tag)
    gvk, gpubs, gproof = GV.golden("groth16_bn128_n1024.json")
    gbad = [str((int(gpubs[0]) + 1) % FV.E.R)] + gpubs[1:]
    pvk, ppubs, pproof = PV.golden(PV.GOLDEN_FILES[0])
    fvk, fpubs, fproof = FV.golden(FV.GOLDEN_FILES[0])
    gkey, pkey, fkey = gv.VerifyingKey(gvk), pv.VerifyingKey(pvk), fv.VerifyingKey(fvk)

    def per_proof():
        return (gkey.verify_codes([gpubs, gbad], [gproof, gproof]),
                pkey.verify_codes([ppubs, ppubs], [pproof, PV.with_(pproof, eval_a=str((int(pproof["eval_a"]) + 1) % FV.E.R))]),
                fkey.verify_codes([fpubs, fpubs], [fproof, FV.with_eval(fproof, "z", (int(fproof["evaluations"]["z"]) + 1) % FV.E.R)]),
                c.key.verify_codes(lists[:70], proofs[:69] + [c.bad_eval(proofs[69])]))
    before = per_proof()
    assert before[:3] == ([1, 0], [1, 0], [1, 0]) and before[3] == [1] * 69 + [0]
    gz, gw = open(os.path.join(gd, "groth16_bn128_n1024.zkey"), "rb").read(), open(os.path.join(gd, "groth16_bn128_n1024.wtns"), "rb").read()
    w = zkmi.u8(binfile.read_wtns(gw)["witness"])
    r_m, s_m = OL.fr_e(OL.BN128, 3), OL.fr_e(OL.BN128, 5)
    d = zkmi.C.c_void_p(0)
    zkmi.check(L.zkmi_dev_alloc(w.size, zkmi.C.byref(d)))
    zkmi.check(L.zkmi_memcpy_h2d(d, zkmi.ptr(w), w.size))
    pk = groth16.ProvingKey(gz)
    try:
        pk.submit(d.value, 0)
        gref = [bytes(x) for x in pk.collect(0, r_m, s_m)]
        for slot in (0, 1):
            pk.submit(d.value, slot)
            ok, codes = c.key.verify_all_raw(recs, pb, n_sig, n, seed)
            assert ok and (codes == 1).all()
            assert [bytes(x) for x in pk.collect(slot, r_m, s_m)] == gref, slot
        assert per_proof() == before
    finally:
        for k in (gkey, pkey, fkey):
            k.release()
        pk.release()
        L.zkmi_dev_free(d)
