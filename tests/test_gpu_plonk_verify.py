"""Batch PLONK verification on the device (csrc/plonk_verify.hip) against the reference's verdicts. Every expectation comes from
tests/plonk_verify_vectors.py (oracle/plonk_verify_oracle.py::verifier_values + the pairing of oracle/groth16_verify_oracle.py, checked on
the CPU by tests/test_plonk_verify_host.py) or, for keys too large for the pure-Python MSM to be quick, from the oracle's verify_known_tau:
golden proofs, the device's trace, tampers, device-proved synthetic keys up to 2^20, mixed batches with exact verdict arrays, and provers
left untouched by a verify batch."""
import os
import random
import threading

import pytest

import plonk_verify_oracle as PO
import plonk_verify_vectors as V

pytestmark = pytest.mark.gpu
_expected = {}


def expected(tag, vk, pubs, proof):
    if tag not in _expected:
        _expected[tag] = V.expected_code(vk, pubs, proof)
    return _expected[tag]


@pytest.fixture(scope="module")
def pv():
    from snarkjs_amd import plonk_verify
    return plonk_verify


class Log:
    def __init__(self):
        self.lines = []

    def _add(level):
        return lambda self, m: self.lines.append((level, m))
    debug, info, warn, error = _add("debug"), _add("info"), _add("warn"), _add("error")


def check_trace(got, want):
    for k in ("beta", "gamma", "alpha", "xi", "u", "pi", "r0", "A1", "B1"):
        assert got[k] == want[k], k
    assert got["v1"] == want["v"][1] and got["L1"] == want["L"][1]


@pytest.mark.parametrize("f", V.GOLDEN_FILES)
def test_golden_trace_and_tampers(pv, f):
    import json
    vk, pubs, proof = V.golden(f)
    key = pv.VerifyingKey(vk)
    # the device's intermediate values: the reference verifier's own trace (beta ... r0) and verifier_values
    tr = key.trace(pubs, proof)
    check_trace(tr, V.values(vk, pubs, proof))
    ref = json.load(open(os.path.join(V.GOLDEN, f)))["verify_trace"]
    by = {}
    for line in ref:                                            # "beta: <hex>", five "v: <hex>" (v1 first), "L1(xi)=<hex>", "PI(xi): <hex>", ...
        name, val = line.split("=", 1) if line.startswith("L") else line.split(": ", 1)
        by.setdefault(name, val)
    for name, k in (("beta", "beta"), ("gamma", "gamma"), ("alpha", "alpha"), ("xi", "xi"), ("v", "v1"), ("u", "u"), ("L1(xi)", "L1"), ("PI(xi)", "pi"), ("r0", "r0")):
        assert int(by[name], 16) == tr[k], name
    cases = [("golden", pubs, proof, 1)] + V.tampers(vk, pubs, proof)
    by_count = {}
    for c in cases:
        by_count.setdefault(len(c[1]), []).append(c)
    for n_sig, group in by_count.items():
        got = key.verify_codes([c[1] for c in group], [c[2] for c in group])
        for (label, pu, p, want), g in zip(group, got):
            if want is None:
                want = expected((f, label), vk, pu, p)
            assert g == want, label
    # the drop-in call: return value and logger messages of the reference
    E = V.curve_of(vk)
    bad_point = V.with_(proof, A=[str(int(proof["A"][0]) + 1), proof["A"][1], "1"])
    for pu, p, code in ((pubs, proof, 1), (pubs, V.with_(proof, eval_c=str((int(proof["eval_c"]) + 1) % E.R)), 0), ([str(E.R)] + pubs[1:], proof, -1),
                        (pubs, bad_point, -2), (pubs + ["1"], proof, -3)):
        log = Log()
        assert pv.verify(vk, pu, p, log) is (code == 1)
        assert log.lines == [("info", "PLONK VERIFIER STARTED"), V.MESSAGES[code]]
    assert pv.verify(vk, pubs, bad_point) is False              # the reference throws here without a logger: False instead
    assert pv.verify(vk, pubs, proof) is True
    pv.release_all()
    key.release()


@pytest.mark.parametrize("f", V.GOLDEN_FILES)
@pytest.mark.parametrize("n", [0, 1, 40])
def test_other_public_counts(pv, f, n):
    """a golden proof under a key with another nPublic is invalid, yet every intermediate value and the verdict are defined"""
    vk, _, proof = V.golden(f)
    v, pu = V.with_n_public(vk, n, 0x70 + n)
    key = pv.VerifyingKey(v)
    check_trace(key.trace(pu, proof), V.values(v, pu, proof))
    assert key.verify_codes([pu], [proof]) == [expected((f, n), v, pu, proof)] == [0]
    key.release()


def test_key_with_qc_at_infinity(pv):
    vk, pubs, proof = V.golden(V.GOLDEN_FILES[0])
    v = dict(vk, Qc=["0", "1", "0"])
    key = pv.VerifyingKey(v)
    check_trace(key.trace(pubs, proof), V.values(v, pubs, proof))
    assert key.verify_codes([pubs], [proof]) == [expected("qc_inf", v, pubs, proof)]
    key.release()
    from snarkjs_amd import zkmi
    with pytest.raises(zkmi.ZkmiError, match="not on the curve"):
        pv.VerifyingKey(dict(vk, Qc=[str(int(vk["Qc"][0]) + 1), vk["Qc"][1], "1"]))


@pytest.mark.parametrize("curve,lg", [("bn128", 6), ("bn128", 10), ("bn128", 13), ("bn128", 16), ("bls12381", 6), ("bls12381", 13), ("bn128", 20)])
def test_device_proved_keys(pv, curve, lg):
    """a synthetic key (nPublic = 1, X_2 = [tau]·G2 in its header) proved by the device prover: the proof verifies on the device with a real
    pairing, one flipped evaluation does not. Expectation: the helper's pairing composition up to 2^10, the oracle's known-tau check beyond."""
    import synth_plonk
    from snarkjs_amd import plonk
    tau = 0x1F3D5B79
    zkey, wtns = synth_plonk.make(curve, lg, seed=11, tau=tau)
    res = plonk.prove(zkey, wtns)
    vk = pv.vk_from_zkey(zkey)
    assert vk["curve"] == curve and vk["nPublic"] == 1 and vk["power"] == lg
    assert vk["Qc"] == ["0", "1", "0"]                          # the synthetic circuit has no constants: a key whose Qc is the point at infinity
    E = V.curve_of(vk)
    pubs, proof = res["publicSignals"], res["proof"]
    bad = V.with_(proof, eval_s1=str((int(proof["eval_s1"]) + 1) % E.R))
    if lg <= 10:
        want = [V.expected_code(vk, pubs, proof), V.expected_code(vk, pubs, bad)]
    else:
        want = [1 if PO.verify_known_tau(vk, pubs, p, tau) else 0 for p in (proof, bad)]
    assert want == [1, 0]
    key = pv.VerifyingKey(vk)
    assert key.verify_codes([pubs, pubs], [proof, bad]) == want
    key.release()


def _mixed_batch(vk, pubs, proof, n, seed):
    """n entries: the golden proof with commitments re-encoded in Jacobian form (a distinct z per entry, so every lane reads different bytes),
    about one in four invalid at seeded positions (an evaluation or a public signal moved by one)"""
    E = V.curve_of(vk)
    rnd = random.Random(seed)
    assert pubs
    lists, proofs, kinds = [], [], []
    for i in range(n):
        k = rnd.choice(V.POINTS)
        p = V.with_(proof, **{k: V.jacobian(E, V.affine(E, proof[k]), 2 + i)})
        kind = rnd.randrange(8)
        if kind == 0:
            p["eval_zw"] = str((int(p["eval_zw"]) + 1) % E.R)
        lists.append([str((int(pubs[0]) + 1) % E.R)] + pubs[1:] if kind == 1 else pubs)
        proofs.append(p)
        kinds.append(min(kind, 2))
    return lists, proofs, kinds


@pytest.mark.parametrize("f,n", [(V.GOLDEN_FILES[0], 1), (V.GOLDEN_FILES[0], 63), (V.GOLDEN_FILES[0], 65), (V.GOLDEN_FILES[1], 4097), (V.GOLDEN_FILES[2], 65)])
def test_batch_exact(pv, f, n):
    vk, pubs, proof = V.golden(f)
    E = V.curve_of(vk)
    lists, proofs, kinds = _mixed_batch(vk, pubs, proof, n, 0xb0 + n)
    # a Jacobian re-encoding names the same point, so a verdict depends on the kind alone: one helper call per kind, eight sampled positions in full
    by_kind = {0: expected((f, "zw+1"), vk, pubs, V.with_(proof, eval_zw=str((int(proof["eval_zw"]) + 1) % E.R))),
               1: expected((f, "pub+1"), vk, [str((int(pubs[0]) + 1) % E.R)] + pubs[1:], proof), 2: expected(f, vk, pubs, proof)}
    assert by_kind == {0: 0, 1: 0, 2: 1}
    key = pv.VerifyingKey(vk)
    got = key.verify_codes(lists, proofs)
    assert got == [by_kind[k] for k in kinds]
    for i in random.Random(2).sample(range(n), min(n, 8)):
        assert got[i] == V.expected_code(vk, lists[i], proofs[i]), i
    recs, pb, n_sig, _ = key.pack(lists, proofs)
    assert [int(c) for c in key.verify_raw(recs, pb, n_sig, n)] == got
    key.release()


def test_batch_of_distinct_device_proofs(pv):
    """66 proofs of one witness with fresh blinding each (two wavefronts whose lanes carry different challenges and scalars), every fifth with one
    evaluation moved: every verdict from the helper"""
    from snarkjs_amd import plonk
    vk, pubs, _ = V.golden(V.GOLDEN_FILES[1])
    E = V.curve_of(vk)
    pkey = plonk.PlonkKey(open(os.path.join(V.GOLDEN, "plonk_bn128_n2048.zkey"), "rb").read())
    wtns = open(os.path.join(V.GOLDEN, "plonk_bn128_n2048.wtns"), "rb").read()
    proofs = [plonk.prove(pkey, wtns)["proof"] for _ in range(66)]
    pkey.release()
    assert len({p["Wxiw"][0] for p in proofs}) == 66
    for i in range(0, 66, 5):
        proofs[i] = V.with_(proofs[i], eval_b=str((int(proofs[i]["eval_b"]) + 1) % E.R))
    want = [V.expected_code(vk, pubs, p) for p in proofs]
    assert want == [0 if i % 5 == 0 else 1 for i in range(66)]
    key = pv.VerifyingKey(vk)
    assert key.verify_codes([pubs] * 66, proofs) == want
    key.release()


def test_provers_in_flight_unaffected(pv):
    """a PLONK proof in flight and a Groth16 proof submitted to each pipeline slot BEFORE a 4 097-proof PLONK verify batch and finished AFTER
    it equal the same proofs with no verify in between"""
    import oracle_lib as OL
    from snarkjs_amd import groth16, binfile, zkmi, plonk
    gd = V.GOLDEN
    vk, pubs, proof = V.golden(V.GOLDEN_FILES[1])
    key = pv.VerifyingKey(vk)
    L = zkmi.lib()
    # PLONK prover: the coroutine stops before each of its blocking calls; the verify batch runs between two of them
    zkey, wtns = open(os.path.join(gd, "plonk_bn128_n2048.zkey"), "rb").read(), open(os.path.join(gd, "plonk_bn128_n2048.wtns"), "rb").read()
    pkey = plonk.PlonkKey(zkey)
    blind = [bytes(pkey.f.mont(9000 + 7 * i)) for i in range(11)]
    ref = plonk.prove(pkey, wtns, blinding_mont=blind)
    for stop_after in (1, 3):
        steps = plonk._prove_steps(pkey, wtns, None, None, blind)
        for _ in range(stop_after):
            next(steps)
        assert key.verify_many([pubs] * 4097, [proof] * 4097) == [True] * 4097
        try:
            while True:
                next(steps)
        except StopIteration as done:
            assert done.value == ref, stop_after
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
            assert key.verify_many([pubs] * 4097, [proof] * 4097) == [True] * 4097
            assert [bytes(x) for x in pk.collect(slot, r_m, s_m)] == gref, slot
    finally:
        key.release()
        pk.release()
        L.zkmi_dev_free(d)


def test_groth16_and_plonk_verify_from_two_threads(pv):
    import verify_vectors as GV
    from snarkjs_amd import groth16_verify as gv
    vk, pubs, proof = V.golden(V.GOLDEN_FILES[0])
    E = V.curve_of(vk)
    gvk, gpubs, gproof = GV.golden("groth16_bn128_n1024.json")
    pkey, gkey = pv.VerifyingKey(vk), gv.VerifyingKey(gvk)
    lists, proofs, kinds = _mixed_batch(vk, pubs, proof, 300, 0x33)
    want_p = [1 if k == 2 else 0 for k in kinds]
    gbad = [str((int(gpubs[0]) + 1) % E.R)] + gpubs[1:]
    glists = [gbad if i % 5 == 0 else gpubs for i in range(300)]
    want_g = [0 if i % 5 == 0 else 1 for i in range(300)]
    out = {}

    def run(name, fn):
        out[name] = [fn() for _ in range(3)]
    ts = [threading.Thread(target=run, args=("p", lambda: pkey.verify_codes(lists, proofs))),
          threading.Thread(target=run, args=("g", lambda: gkey.verify_codes(glists, [gproof] * 300)))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert out["p"] == [want_p] * 3 and out["g"] == [want_g] * 3
    pkey.release()
    gkey.release()
