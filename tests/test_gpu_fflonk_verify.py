"""Batch FFLONK verification on the device (csrc/fflonk_verify.hip) against the reference's verdicts. Every expectation comes from
tests/fflonk_verify_vectors.py (oracle/fflonk_verify_oracle.py::verifier_values + the pairing of oracle/groth16_verify_oracle.py, checked on
the CPU by tests/test_fflonk_verify_host.py) and, for synthetic keys whose SRS has a known tau, from the oracle's verify_known_tau as well:
golden proofs, the device's trace, every tamper, device-proved synthetic keys up to 2^18, mixed batches with exact verdict arrays, a batch of
distinct device proofs, the drop-in verify() with its logger lines, and provers left untouched by a verify batch."""
import os
import random

import pytest

import fflonk_verify_oracle as FO
import fflonk_verify_vectors as V

pytestmark = pytest.mark.gpu
_expected = {}
TAU = 0x1F3D5B79


def expected(tag, vk, pubs, proof):
    if tag not in _expected:
        _expected[tag] = V.expected_code(vk, pubs, proof)
    return _expected[tag]


@pytest.fixture(scope="module")
def fv():
    from snarkjs_amd import fflonk_verify
    return fflonk_verify


class Log:
    def __init__(self):
        self.lines = []

    def _add(level):
        return lambda self, m: self.lines.append((level, m))
    debug, info, warn, error = _add("debug"), _add("info"), _add("warn"), _add("error")


def check_trace(got, want):
    for k in ("beta", "gamma", "xi", "alpha", "y", "r0", "r1", "r2", "A1", "B1"):
        assert got[k] == want[k], k


@pytest.mark.parametrize("f", V.GOLDEN_FILES)
def test_golden_trace_and_every_tamper(fv, f):
    import json
    vk, pubs, proof = V.golden(f)
    key = fv.VerifyingKey(vk)
    tr = key.trace(pubs, proof)
    check_trace(tr, V.values(vk, pubs, proof))
    (nx, ny), (bx, by) = json.load(open(os.path.join(V.GOLDEN, f)))["pairing_inputs"]              # the reference's own arguments of pairingEq: -A1, W2
    assert tr["A1"] == (int(nx), (V.E.P - int(ny)) % V.E.P) and tr["B1"] == (int(bx), int(by))
    cases = [("golden", pubs, proof, 1)] + V.tampers(vk, pubs, proof)
    want = [c[3] if c[3] is not None else expected((f, c[0]), vk, c[1], c[2]) for c in cases]
    assert want[0] == 1 and {1, 0, -1, -2, -3} == set(want)
    by_label = dict(zip([c[0] for c in cases], want))
    assert by_label["a_plus_r"] == 1 and by_label["inv_changed"] == 1 and by_label["bad_point_and_wrong_count"] == -3 and by_label["bad_point_and_bad_public"] == -2
    # singly
    for (label, pu, p, _), w in zip(cases, want):
        assert key.verify_codes([pu], [p]) == [w], label
    # as mixed batches: one per number of signals (a batch carries one count)
    by_count = {}
    for c, w in zip(cases, want):
        by_count.setdefault(len(c[1]), []).append((c, w))
    for n_sig, group in by_count.items():
        got = key.verify_codes([c[1] for c, _ in group], [c[2] for c, _ in group])
        assert got == [w for _, w in group], [c[0] for (c, w), g in zip(group, got) if g != w]
    key.release()
    # C0 off the curve in the key: the key loads, a valid proof gets -2
    bad_vk = V.with_c0_off_curve(vk)
    bkey = fv.VerifyingKey(bad_vk)
    assert bkey.verify_codes([pubs], [proof]) == [expected((f, "c0"), bad_vk, pubs, proof)] == [-2]
    assert bkey.verify_codes([pubs + ["1"]], [proof]) == [-3]                                   # the count still comes first
    bkey.release()


@pytest.mark.parametrize("n", V.N_PUBLIC_CASES)
def test_other_public_counts(fv, n):
    """a golden proof under a key with another nPublic is invalid, yet every intermediate value and the verdict are defined"""
    vk, _, proof = V.golden(V.GOLDEN_FILES[0])
    v, pu = V.with_n_public(vk, n, 0x70 + n)
    key = fv.VerifyingKey(v)
    check_trace(key.trace(pu, proof), V.values(v, pu, proof))
    assert key.verify_codes([pu], [proof]) == [expected(("np", n), v, pu, proof)] == [0]
    key.release()


def test_refused_keys(fv):
    from snarkjs_amd import zkmi
    import numpy as np
    vk, _, _ = V.golden(V.GOLDEN_FILES[0])
    x2 = [list(c) for c in vk["X_2"]]
    x2[0][0] = str(int(x2[0][0]) + 1)
    with pytest.raises(zkmi.ZkmiError, match="X_2 is not on the curve"):
        fv.VerifyingKey(dict(vk, X_2=x2))
    with pytest.raises(ValueError, match="bn128 only"):
        fv.VerifyingKey(dict(vk, curve="bls12381"))
    z = np.zeros(1024, np.uint8)
    h = zkmi.C.c_uint64(0)
    assert zkmi.lib().zkmi_fflonk_vk_load(zkmi.BLS12381, zkmi.ptr(z), zkmi.ptr(z), zkmi.ptr(z), 3, 1, zkmi.C.byref(h)) != 0
    assert b"BN254 only" in zkmi.lib().zkmi_last_error()


@pytest.mark.parametrize("lg", [12, 16, 18])
def test_device_proved_keys(fv, lg):
    """a synthetic key (nPublic = 1, X_2 = [tau]·G2 in its header) proved by the device prover, vk from vk_from_zkey: the proof verifies on the
    device with a real pairing, one flipped evaluation does not; both as the oracle's known-tau check has them"""
    import synth_plonk
    from snarkjs_amd import fflonk
    zkey, wtns = synth_plonk.make_fflonk(lg, seed=5, tau=TAU)
    res = fflonk.prove(zkey, wtns)
    vk = fv.vk_from_zkey(zkey)
    ovk = FO.vk_from_zkey(zkey)
    assert vk["nPublic"] == 1 and vk["power"] == lg and all(str(vk[k]) == str(ovk[k]) for k in ovk)
    pubs, proof = res["publicSignals"], res["proof"]
    bad = V.with_eval(proof, "s2", (int(proof["evaluations"]["s2"]) + 1) % V.E.R)
    want = [1 if FO.verify_known_tau(vk, pubs, p, TAU) else 0 for p in (proof, bad)]
    assert want == [1, 0]
    if lg == 12:
        assert [V.expected_code(vk, pubs, proof), V.expected_code(vk, pubs, bad)] == want
    key = fv.VerifyingKey(vk)
    assert key.verify_codes([pubs, pubs], [proof, bad]) == want
    key.release()


def _mixed_batch(vk, pubs, proof, n, seed):
    """n entries: the golden proof with one commitment re-encoded in Jacobian form (a distinct z per entry, so every lane reads different bytes),
    about three in eight invalid at seeded positions (an evaluation or a public signal moved by one, a point off the curve)"""
    rnd = random.Random(seed)
    lists, proofs, kinds = [], [], []
    for i in range(n):
        k = rnd.choice(V.POINTS)
        p = V.with_point(proof, k, V.jacobian(V.affine(proof["polynomials"][k]), 2 + i))
        kind = rnd.randrange(8)
        if kind == 0:
            p["evaluations"]["zw"] = str((int(p["evaluations"]["zw"]) + 1) % V.E.R)
        if kind == 2:
            p["polynomials"]["W1"] = V.off_curve(proof["polynomials"]["W1"])
        lists.append([str((int(pubs[0]) + 1) % V.E.R)] + pubs[1:] if kind == 1 else pubs)
        proofs.append(p)
        kinds.append(min(kind, 3))
    return lists, proofs, kinds


@pytest.mark.parametrize("f,n", [(V.GOLDEN_FILES[0], 1), (V.GOLDEN_FILES[0], 63), (V.GOLDEN_FILES[1], 65), (V.GOLDEN_FILES[1], 257)])
def test_batch_exact(fv, f, n):
    vk, pubs, proof = V.golden(f)
    lists, proofs, kinds = _mixed_batch(vk, pubs, proof, n, 0xb0 + n)
    # a Jacobian re-encoding names the same point, so a verdict depends on the kind alone: one helper call per kind, eight sampled positions in full
    by_kind = {0: expected((f, "zw_plus_1"), vk, pubs, V.with_eval(proof, "zw", (int(proof["evaluations"]["zw"]) + 1) % V.E.R)),
               1: expected((f, "public0_plus_1"), vk, [str((int(pubs[0]) + 1) % V.E.R)] + pubs[1:], proof), 2: -2, 3: expected(f, vk, pubs, proof)}
    assert by_kind == {0: 0, 1: 0, 2: -2, 3: 1}
    key = fv.VerifyingKey(vk)
    got = key.verify_codes(lists, proofs)
    assert got == [by_kind[k] for k in kinds]
    for i in random.Random(2).sample(range(n), min(n, 8)):
        assert got[i] == V.expected_code(vk, lists[i], proofs[i]), i
    recs, pb, n_sig, _ = key.pack(lists, proofs)
    assert [int(c) for c in key.verify_raw(recs, pb, n_sig, n)] == got
    from snarkjs_amd import zkmi
    with pytest.raises(zkmi.ZkmiError, match="Number of public signals does not match with vk"):
        key.verify_raw(recs, pb[:32 * n * (n_sig - 1)], n_sig - 1, n)
    key.release()


def test_batch_of_distinct_device_proofs(fv):
    """256 proofs of one witness by fflonk.prove_many, fresh blinding each (four wavefronts whose lanes carry different challenges and scalars),
    every seventh with one evaluation moved and every 50th with a public signal moved: every verdict from the oracle's known-tau check, sixteen
    of them from the pairing helper as well"""
    import synth_plonk
    from snarkjs_amd import fflonk
    zkey, wtns = synth_plonk.make_fflonk(12, seed=9, tau=TAU)
    vk = fv.vk_from_zkey(zkey)
    res = fflonk.prove_many(zkey, [wtns] * 256)
    pubs = res[0]["publicSignals"]
    proofs = [r["proof"] for r in res]
    assert len({p["polynomials"]["W2"][0] for p in proofs}) == 256
    lists = [pubs] * 256
    for i in range(0, 256, 7):
        k = V.EVALS[i % 15]
        proofs[i] = V.with_eval(proofs[i], k, (int(proofs[i]["evaluations"][k]) + 1) % V.E.R)
    for i in range(1, 256, 50):
        lists[i] = [str((int(pubs[0]) + 1) % V.E.R)]
    want = [1 if FO.verify_known_tau(vk, pu, p, TAU) else 0 for pu, p in zip(lists, proofs)]
    assert want == [0 if i % 7 == 0 or i % 50 == 1 else 1 for i in range(256)]
    for i in range(0, 256, 16):
        assert V.expected_code(vk, lists[i], proofs[i]) == want[i], i
    key = fv.VerifyingKey(vk)
    assert key.verify_codes(lists, proofs) == want
    key.release()


def test_verify_logger_and_resident_keys(fv):
    """the drop-in call: return value and logger lines (level, message) of the reference: STARTED first, FINISHED only after a pairing verdict"""
    vk, pubs, proof = V.golden(V.GOLDEN_FILES[0])
    bad_point = V.with_point(proof, "C1", V.off_curve(proof["polynomials"]["C1"]))
    for pu, p, code in ((pubs, proof, 1), (pubs, V.with_eval(proof, "c", (int(proof["evaluations"]["c"]) + 1) % V.E.R), 0), ([str(V.E.R)] + pubs[1:], proof, -1),
                        (pubs, bad_point, -2), (pubs + ["1"], proof, -3), (pubs + ["1"], bad_point, -3)):
        log = Log()
        assert fv.verify(vk, pu, p, log) is (code == 1)
        assert log.lines == [V.STARTED, V.MESSAGES[code]] + ([V.FINISHED] if code in (0, 1) else []), code
        assert fv.MESSAGES[code] == V.MESSAGES[code][1]
    assert len(fv._resident) == 1                                # one key for the six calls
    handle = next(iter(fv._resident.values())).handle
    assert fv.verify(vk, pubs + ["1"], proof) is False           # the reference throws here without a logger: False instead
    assert fv.verify(vk, pubs, proof) is True
    assert next(iter(fv._resident.values())).handle == handle
    fv.release_all()
    assert not fv._resident
    assert fv.verify(vk, pubs, proof) is True                    # loads again
    fv.release_all()


def test_provers_in_flight_unaffected(fv):
    """fflonk.prove_many's driver with two proofs in flight, a 4 097-proof verify batch issued between their steps, and a Groth16 proof
    submitted to each pipeline slot BEFORE such a batch and finished AFTER it: proofs and verdicts equal the serial ones"""
    import oracle_lib as OL
    from snarkjs_amd import groth16, binfile, zkmi, fflonk
    from snarkjs_amd.plonk import run_many
    gd = V.GOLDEN
    vk, pubs, proof = V.golden(V.GOLDEN_FILES[1])
    key = fv.VerifyingKey(vk)
    L = zkmi.lib()
    bad = V.with_eval(proof, "t1w", (int(proof["evaluations"]["t1w"]) + 1) % V.E.R)
    batch_p = [bad if i % 1000 == 7 else proof for i in range(4097)]
    serial = key.verify_codes([pubs] * 4097, batch_p)
    assert serial == [expected("iso_bad", vk, pubs, bad) if i % 1000 == 7 else expected("iso", vk, pubs, proof) for i in range(4097)]
    assert serial[7] == 0 and serial[0] == 1
    zkey, wtns = open(os.path.join(gd, "fflonk_bn128_n256.zkey"), "rb").read(), open(os.path.join(gd, "fflonk_bn128_n256.wtns"), "rb").read()
    pkey = fflonk.FflonkKey(zkey)
    blinds = [[bytes(pkey.f.mont(9000 + 100 * j + 7 * i)) for i in range(9)] for j in range(3)]
    ref = fflonk.prove_many(pkey, [wtns] * 3, blinds)
    assert ref == [fflonk.prove(pkey, wtns, blinding_mont=b) for b in blinds]
    verified = []

    def steps_with_verify(i):
        steps = fflonk._prove_steps(pkey, wtns, None, None, blinds[i])
        k = 0
        try:
            while True:
                next(steps)
                k += 1
                if (i, k) in ((0, 2), (1, 4), (2, 1)):          # the other proof of the pair is in flight on its own slot
                    verified.append(key.verify_codes([pubs] * 4097, batch_p) == serial)
                yield
        except StopIteration as done:
            return done.value
    assert run_many(steps_with_verify, 3) == ref
    assert verified == [True] * 3
    pkey.release()
    # Groth16 prover, each pipeline slot
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
            assert key.verify_codes([pubs] * 4097, batch_p) == serial
            assert [bytes(x) for x in pk.collect(slot, r_m, s_m)] == gref, slot
    finally:
        key.release()
        pk.release()
        L.zkmi_dev_free(d)


def test_groth16_and_plonk_verifiers_after_an_fflonk_batch(fv):
    """the three verifiers in one process: Groth16 and PLONK give the verdicts of their own goldens and tampers after an FFLONK batch"""
    import plonk_verify_vectors as PV
    import verify_vectors as GV
    from snarkjs_amd import groth16_verify as gv, plonk_verify as pv
    vk, pubs, proof = V.golden(V.GOLDEN_FILES[0])
    key = fv.VerifyingKey(vk)
    bad = V.with_eval(proof, "qm", (int(proof["evaluations"]["qm"]) + 1) % V.E.R)
    want_f = [expected(V.GOLDEN_FILES[0], vk, pubs, proof), expected("qm_bad", vk, pubs, bad)] * 100
    assert want_f[:2] == [1, 0]
    pvk, ppubs, pproof = PV.golden(PV.GOLDEN_FILES[0])
    pbad = PV.with_(pproof, eval_a=str((int(pproof["eval_a"]) + 1) % V.E.R))
    want_p = [PV.expected_code(pvk, ppubs, pproof), PV.expected_code(pvk, ppubs, pbad)]
    gvk, gpubs, gproof = GV.golden("groth16_bn128_n1024.json")
    gbad = [str((int(gpubs[0]) + 1) % V.E.R)] + gpubs[1:]
    pkey, gkey = pv.VerifyingKey(pvk), gv.VerifyingKey(gvk)
    before = (pkey.verify_codes([ppubs, ppubs], [pproof, pbad]), gkey.verify_codes([gpubs, gbad], [gproof, gproof]))
    assert before == (want_p, [1, 0]) and want_p == [1, 0]
    assert key.verify_codes([pubs] * 200, [proof, bad] * 100) == want_f
    after = (pkey.verify_codes([ppubs, ppubs], [pproof, pbad]), gkey.verify_codes([gpubs, gbad], [gproof, gproof]))
    assert after == before
    assert key.verify_codes([pubs] * 200, [proof, bad] * 100) == want_f
    for k in (key, pkey, gkey):
        k.release()
