"""The aggregated Groth16 check on the device (groth16_verify.VerifyingKey.verify_all / verify_all_raw / verify_many_fast / aggregate_trace) against
the per-proof verifier of the same key and against tests/groth16_aggregate_vectors.py: verify_all == all(code == 1 for code in verify_codes) on
batches of distinct device proofs (a distinct (r, s) each, so every pi_b differs) with and without one tampered member and with each structural
failure, a pair of tampers that cancels without the challenges, encodings and points at infinity, keys with 0 / 2 / 40 publics, fewer signals
than nPublic, the trace against the Python restatement, the timers, and the isolation rules of the per-proof verifiers."""
import copy
import os
import random
import time

import numpy as np
import pytest

import groth16_aggregate_vectors as GA
import groth16_verify_oracle as O
import verify_vectors as GV

pytestmark = pytest.mark.gpu
SIZES = {"groth16_bn128_n1024": (1, 63, 64, 65, 4096, 4097), "groth16_bls12381_n1024": (1, 65, 1024)}
CASES = [(tag, n) for tag, sizes in SIZES.items() for n in sizes]


class Case:
    """one golden key: the resident key, max(SIZES) distinct device proofs of the golden witness (a distinct (r, s) each), the tampers"""

    def __init__(self, tag):
        import oracle_lib as OL
        from snarkjs_amd import groth16, binfile, zkmi, groth16_verify
        self.tag = tag
        self.vk, self.pubs, self.golden = GV.golden(tag + ".json")
        self.E = GA.curve_of(self.vk)
        zkey = open(os.path.join(GV.GOLDEN, tag + ".zkey"), "rb").read()
        wtns = open(os.path.join(GV.GOLDEN, tag + ".wtns"), "rb").read()
        w = zkmi.u8(binfile.read_wtns(wtns)["witness"])
        curve = OL.BN128 if self.vk["curve"] == "bn128" else OL.BLS12381
        L = zkmi.lib()
        d = zkmi.C.c_void_p(0)
        zkmi.check(L.zkmi_dev_alloc(w.size, zkmi.C.byref(d)))
        zkmi.check(L.zkmi_memcpy_h2d(d, zkmi.ptr(w), w.size))
        pk = groth16.ProvingKey(zkey)
        n = max(SIZES[tag])
        try:
            raw = []
            pk.submit(d.value, 0)
            for i in range(n):
                if i + 1 < n:
                    pk.submit(d.value, (i + 1) & 1)
                raw.append([x.copy() for x in pk.collect(i & 1, OL.fr_e(curve, 3 + 2 * i), OL.fr_e(curve, 4 + 2 * i))])
            self.proofs = [groth16.raw_to_proof(pk, *r) for r in raw]
        finally:
            pk.release()
            L.zkmi_dev_free(d)
        assert len({tuple(p["pi_b"][0]) for p in self.proofs}) == n            # the pi_b are distinct
        self.key = groth16_verify.VerifyingKey(self.vk)
        self.alpha = GA.alpha_of(self.E, self.vk)

    def bad_c(self, p, sign=1):
        return GA.with_c_plus(self.E, p, self.alpha, sign)

    def off_curve(self, p):
        q = copy.deepcopy(p)
        q["pi_a"][0] = str((int(q["pi_a"][0]) + 1) % self.E.P)
        return q


_cases = {}


def case_of(tag):
    if tag not in _cases:
        _cases[tag] = Case(tag)
    return _cases[tag]


@pytest.fixture(params=list(SIZES), ids=list(SIZES))
def case(request):
    return case_of(request.param)


def agree(key, lists, proofs, seed):
    """verify_all, verify_many_fast and the per-proof verifier on one batch; returns the per-proof codes"""
    codes = key.verify_codes(lists, proofs)
    assert key.verify_all(lists, proofs, seed) == all(x == 1 for x in codes)
    assert key.verify_many_fast(lists, proofs, seed) == key.verify_many(lists, proofs) == [x == 1 for x in codes]
    return codes


@pytest.mark.parametrize("tag,n", CASES)
def test_equivalence(tag, n):
    c = case_of(tag)
    rnd = random.Random("g16 eq %s %d" % (tag, n))
    seed = GA.seed_of("g16 eq %s %d" % (tag, n))
    proofs, lists = c.proofs[:n], [c.pubs] * n
    assert agree(c.key, lists, proofs, seed) == [1] * n
    assert c.key.verify_all(lists, proofs) is True                               # a seed from the OS
    at = rnd.randrange(n)
    tampered = proofs[:at] + [c.bad_c(proofs[at])] + proofs[at + 1:]
    assert agree(c.key, lists, tampered, seed) == [0 if i == at else 1 for i in range(n)]
    recs, pb, n_sig, _ = c.key.pack(lists, tampered)
    ok, codes = c.key.verify_all_raw(recs, pb, n_sig, n, seed)
    assert not ok and [int(x) for x in codes] == [1] * n
    # each structural failure: pi_a off the curve (-2), a public signal equal to r (-1: caught while packing, and on the device)
    at = rnd.randrange(n)
    off = proofs[:at] + [c.off_curve(proofs[at])] + proofs[at + 1:]
    assert agree(c.key, lists, off, seed) == [-2 if i == at else 1 for i in range(n)]
    recs, pb, n_sig, _ = c.key.pack(lists, off)
    ok, codes = c.key.verify_all_raw(recs, pb, n_sig, n, seed)
    assert not ok and [int(x) for x in codes] == [-2 if i == at else 1 for i in range(n)]
    assert c.pubs
    big = lists[:at] + [[str(c.E.R)] + list(c.pubs[1:])] + lists[at + 1:]
    assert agree(c.key, big, proofs, seed) == [-1 if i == at else 1 for i in range(n)]
    recs, pb, n_sig, _ = c.key.pack(lists, proofs)
    pb = pb.copy()
    pb[32 * len(c.pubs) * at:32 * len(c.pubs) * at + 32] = np.frombuffer(int(c.E.R).to_bytes(32, "little"), np.uint8)
    ok, codes = c.key.verify_all_raw(recs, pb, n_sig, n, seed)
    assert not ok and [int(x) for x in codes] == [-1 if i == at else 1 for i in range(n)]
    assert [int(x) for x in c.key.verify_raw(recs, pb, n_sig, n)] == [-1 if i == at else 1 for i in range(n)]


def test_cancelling_pair(case):
    """pi_c + T in one proof and pi_c - T in another: the unweighted product of the two checks is one, so only the challenges reject the batch"""
    c = case
    n = 70
    proofs, lists = list(c.proofs[:n]), [c.pubs] * n
    proofs[3], proofs[66] = c.bad_c(proofs[3], 1), c.bad_c(proofs[66], -1)
    assert c.key.verify_codes(lists, proofs) == [0 if i in (3, 66) else 1 for i in range(n)]
    for tagged in ("cancel 1", "cancel 2"):
        assert c.key.verify_all(lists, proofs, GA.seed_of(tagged + c.tag)) is False


def test_encodings_and_infinity(case):
    c = case
    seed = GA.seed_of("g16 enc " + c.tag)
    n = 66
    proofs = [GV.jacobian(c.E, p, 2 + i, 3 + i) if i % 3 else p for i, p in enumerate(c.proofs[:n])]
    lists = [c.pubs] * n
    assert agree(c.key, lists, proofs, seed) == [1] * n
    for k, inf in (("pi_a", ["0", "1", "0"]), ("pi_b", [["0", "0"], ["1", "0"], ["0", "0"]]), ("pi_c", ["0", "1", "0"])):
        bad = list(proofs)
        bad[5] = dict(proofs[5], **{k: inf})
        codes = agree(c.key, lists, bad, seed)
        assert codes[:5] + codes[6:] == [1] * (n - 1) and codes[5] == GV.oracle_verdict(c.E, c.vk, c.pubs, bad[5])
        # alone in a batch: whatever the per-proof check says
        agree(c.key, [c.pubs], [bad[5]], seed)


def _trapdoor_key(E, base_vk, n_public, seed):
    """a verifying key with nPublic = n_public and a valid proof for random publics: IC_i = k_i alpha_1, delta = gamma, A = alpha_1,
    B = beta_2, C = -vk_x (then e(-A, B) e(alpha, beta) = 1 and e(vk_x, gamma) e(C, gamma) = 1)"""
    rnd = random.Random(seed)
    al = O._g1(base_vk["vk_alpha_1"])
    ic = [E.g1_mul(al, rnd.randrange(1, E.R)) for _ in range(n_public + 1)]
    vk = dict(base_vk)
    vk["nPublic"] = n_public
    vk["vk_delta_2"] = base_vk["vk_gamma_2"]
    vk["IC"] = [[str(p[0]), str(p[1]), "1"] for p in ic]
    pubs = [str(rnd.randrange(E.R)) for _ in range(n_public)]
    vx = ic[0]
    for v, p in zip(pubs, ic[1:]):
        vx = E.g1_add(vx, E.g1_mul(p, int(v)))
    c = E.g1_neg(vx)
    proof = {"pi_a": base_vk["vk_alpha_1"], "pi_b": base_vk["vk_beta_2"], "pi_c": ["0", "1", "0"] if c is None else [str(c[0]), str(c[1]), "1"]}
    return vk, pubs, proof


@pytest.mark.parametrize("f", ["groth16_bn128_n1024.json", "groth16_bls12381_n1024.json"])
@pytest.mark.parametrize("n_public", [0, 2, 40])
def test_public_counts(f, n_public):
    from snarkjs_amd import groth16_verify
    base, _, _ = GV.golden(f)
    E = GA.curve_of(base)
    vk, pubs, proof = _trapdoor_key(E, base, n_public, 0x77 + n_public)
    key = groth16_verify.VerifyingKey(vk)
    seed = GA.seed_of("g16 np %d" % n_public)
    try:
        good = [proof, GV.jacobian(E, proof, 3, 5), proof]
        assert agree(key, [pubs] * 3, good, seed) == [1] * 3
        if n_public:
            lists = [pubs, pubs[:-1] + [str((int(pubs[-1]) + 1) % E.R)], pubs]
            assert agree(key, lists, good, seed) == [1, 0, 1]
        ok, codes, sx, sc, s, _ = key.aggregate_trace([pubs] * 3, good, seed)
        want = GA.restate(vk, [(pubs, p) for p in good], seed, pairing=False)
        assert ok and ([int(x) for x in codes], sx, sc, s) == want[1:5]
    finally:
        key.release()


def test_fewer_signals_than_n_public():
    from snarkjs_amd import groth16_verify
    base, _, _ = GV.golden("groth16_bn128_n1024.json")
    E = O.BN254
    vk, pubs, proof = _trapdoor_key(E, base, 5, 0x5)
    vx = O._g1(vk["IC"][0])
    for v, p in zip(pubs[:3], vk["IC"][1:4]):
        vx = E.g1_add(vx, E.g1_mul(O._g1(p), int(v)))
    c = E.g1_neg(vx)
    proof3 = dict(proof, pi_c=[str(c[0]), str(c[1]), "1"])
    key = groth16_verify.VerifyingKey(vk)
    seed = GA.seed_of("g16 fewer")
    try:
        assert agree(key, [pubs[:3]] * 2, [proof3, GV.jacobian(E, proof3, 3, 5)], seed) == [1, 1]
        assert agree(key, [pubs[:3]] * 2, [proof3, proof], seed) == [1, GV.oracle_verdict(E, vk, pubs[:3], proof)]
    finally:
        key.release()


def test_wrong_signal_count_and_empty_batch(case):
    from snarkjs_amd import zkmi
    c = case
    more = [list(c.pubs) + ["1"]] * 3
    with pytest.raises(ValueError, match="nPublic"):
        c.key.verify_all(more, c.proofs[:3])
    recs, _, _, _ = c.key.pack([c.pubs] * 3, c.proofs[:3])
    pb = np.zeros(3 * 32 * (len(c.pubs) + 1), np.uint8)
    for call in (c.key.verify_raw, lambda *a: c.key.verify_all_raw(*a, GA.seed_of("count"))):
        with pytest.raises(zkmi.ZkmiError, match="more public signals than the key's nPublic"):
            call(recs, pb, len(c.pubs) + 1, 3)
    assert c.key.verify_all([], []) is True and c.key.verify_many_fast([], []) == []
    ok, codes = c.key.verify_all_raw(np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    assert ok and codes.size == 0
    assert c.key.aggregate_trace([], [], GA.seed_of("empty")) [2:] == (None, None, 0, list(c.E.F12_ONE))


def test_trace_and_reproducibility(case):
    c = case
    n = 65
    proofs, lists = c.proofs[100:100 + n], [c.pubs] * n
    s1, s2 = GA.seed_of("g16 trace 1 " + c.tag), GA.seed_of("g16 trace 2 " + c.tag)
    ok, codes, sx, sc, s, gt = c.key.aggregate_trace(lists, proofs, s1)
    want = GA.restate(c.vk, list(zip(lists, proofs)), s1, pairing=False)
    assert ok and ([int(x) for x in codes], sx, sc, s) == want[1:5] and sx is not None and sc is not None
    assert c.key.aggregate_trace(lists, proofs, s1)[2:] == (sx, sc, s, gt)
    ok2, _, sx2, sc2, s_2, gt2 = c.key.aggregate_trace(lists, proofs, s2)
    assert ok2 and sx2 != sx and sc2 != sc and s_2 != s and gt2 != gt
    # a tampered member and a structural failure: the sums of the restatement, ok false under both seeds
    bad = proofs[:7] + [c.bad_c(proofs[7])] + proofs[8:40] + [c.off_curve(proofs[40])] + proofs[41:]
    got = c.key.aggregate_trace(lists, bad, s1)
    want = GA.restate(c.vk, list(zip(lists, bad)), s1, pairing=False)
    assert not got[0] and ([int(x) for x in got[1]], got[2], got[3], got[4]) == want[1:5]
    assert not c.key.aggregate_trace(lists, bad, s2)[0]


def test_trace_gt(case):
    """final_exp of the product of the lanes' Miller values, and the verdict, against the restatement's Python pairings: 5 proofs, accept and reject"""
    c = case
    seed = GA.seed_of("g16 gt " + c.tag)
    proofs, lists = c.proofs[200:205], [c.pubs] * 5
    t0 = time.time()
    for batch in (proofs, proofs[:2] + [c.bad_c(proofs[2])] + proofs[3:]):
        ok, codes, sx, sc, s, gt = c.key.aggregate_trace(lists, batch, seed)
        want = GA.restate(c.vk, list(zip(lists, batch)), seed)
        assert (ok, [int(x) for x in codes], sx, sc, s, gt) == (want[0], want[1], want[2], want[3], want[4], list(want[5]))
        assert ok == (batch is proofs)
    print("two restatements with their Python pairings: %.1f s" % (time.time() - t0))


def test_timers_report_the_aggregated_kernels(case):
    from snarkjs_amd import zkmi
    c = case
    L = zkmi.lib()
    assert c.key.verify_all([c.pubs] * 130, c.proofs[:130], GA.seed_of("ms"))
    ms = (zkmi.C.c_double * 3)()
    zkmi.check(L.zkmi_groth16_aggregate_phase_ms(ms))
    total = L.zkmi_groth16_verify_last_ms()
    assert all(x > 0 for x in ms) and total >= sum(ms) * 0.99
    c.key.verify_codes([c.pubs], c.proofs[:1])
    zkmi.check(L.zkmi_groth16_aggregate_phase_ms(ms))
    assert list(ms) == [-1.0] * 3 and L.zkmi_groth16_verify_last_ms() > 0


def test_isolation():
    """a Groth16 proof submitted to each pipeline slot BEFORE a 4 097-proof aggregated Groth16 batch and finished AFTER it keeps its bytes, and the
    three per-proof verifiers and the two KZG verify_all give the same answers before and after"""
    import fflonk_verify_vectors as FV
    import oracle_lib as OL
    import plonk_verify_vectors as PV
    from snarkjs_amd import groth16, binfile, zkmi, plonk_verify as pv, fflonk_verify as fv
    c = case_of("groth16_bn128_n1024")
    L = zkmi.lib()
    n = 4097
    lists, proofs = [c.pubs] * n, c.proofs[:n]
    recs, pb, n_sig, _ = c.key.pack(lists, proofs)
    seed = GA.seed_of("g16 iso")
    gbad = [str((int(c.pubs[0]) + 1) % c.E.R)] + c.pubs[1:]
    pvk, ppubs, pproof = PV.golden(PV.GOLDEN_FILES[0])
    fvk, fpubs, fproof = FV.golden(FV.GOLDEN_FILES[0])
    pkey, fkey = pv.VerifyingKey(pvk), fv.VerifyingKey(fvk)
    pbad = PV.with_(pproof, eval_a=str((int(pproof["eval_a"]) + 1) % FV.E.R))
    fbad = FV.with_eval(fproof, "z", (int(fproof["evaluations"]["z"]) + 1) % FV.E.R)

    def others():
        return (c.key.verify_codes([c.pubs, gbad], [c.golden, c.golden]),
                pkey.verify_codes([ppubs, ppubs], [pproof, pbad]), fkey.verify_codes([fpubs, fpubs], [fproof, fbad]),
                pkey.verify_all([ppubs, ppubs], [pproof, pproof], seed), pkey.verify_all([ppubs, ppubs], [pproof, pbad], seed),
                fkey.verify_all([fpubs, fpubs], [fproof, fproof], seed), fkey.verify_all([fpubs, fpubs], [fproof, fbad], seed))
    before = others()
    assert before == ([1, 0], [1, 0], [1, 0], True, False, True, False)
    gz, gw = open(os.path.join(GV.GOLDEN, "groth16_bn128_n1024.zkey"), "rb").read(), open(os.path.join(GV.GOLDEN, "groth16_bn128_n1024.wtns"), "rb").read()
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
        assert others() == before
    finally:
        for k in (pkey, fkey):
            k.release()
        pk.release()
        L.zkmi_dev_free(d)
