"""The aggregated PLONK / FFLONK check (csrc/kzg_aggregate.cuh) and the chain final exponentiation (csrc/pairing.cuh final_exp_chain) on the CPU
(tools/aggregate_verify_hosttest.hip, the same source with __device__ defined away) against tests/aggregate_verify_vectors.py, which restates
them from the pinned oracles: the chain equals final_exp to the documented power K on both curves, the challenges r_i, the two sums to the
byte, and the verdicts (accepted batches, one tamper at the first / a middle / the last position, every structural failure, the empty
batch). Also the host-only parts of verify_all. No GPU needed; the new entry points must still refuse to run without one.

The host pairing at -O0 takes seconds, so batches stay at or below 8 and seeds are fixed."""
import math
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import aggregate_verify_vectors as AV
import fflonk_verify_vectors as FV
import groth16_verify_oracle as GO
import plonk_verify_vectors as PV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "bin", "aggregate_verify_hosttest")
SRC = os.path.join(ROOT, "tools", "aggregate_verify_hosttest.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "snarkjs_amd", "csrc")
CURVE_ID = {"bn128": 0, "bls12381": 1}


@pytest.fixture(scope="module")
def tool():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("kzg_aggregate.cuh", "plonk_verify.cuh", "fflonk_verify.cuh", "kzg_verify.cuh", "pairing.cuh", "pairing_host.hpp", "curve.cuh",
                                                    "field.cuh", "host_field.hpp")]
    if not os.path.exists(TOOL) or any(os.path.getmtime(d) > os.path.getmtime(TOOL) for d in deps):
        os.makedirs(os.path.dirname(TOOL), exist_ok=True)
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O0", "-std=c++17", "-I" + CSRC, SRC, "-o", TOOL])
    p = subprocess.Popen([TOOL], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)

    def call(*args):
        p.stdin.write(" ".join(str(a) for a in args) + "\n")
        p.stdin.flush()
        out = p.stdout.readline().split()
        assert out and out[0] != "ERR", out
        return out
    yield call
    p.stdin.close()
    p.wait()


def H(v):
    return "%x" % int(v)


def f12(tool, op, ci, f):
    return [int(x, 16) for x in tool(op, ci, *[H(c) for c in f])]


def g2_gen(name):
    return PV.G2_GEN[name]


def miller(tool, E, ci, name, a, b):
    """the code's Miller value of (a G1, b G2) for the generators"""
    g1 = (1, 2) if name == "bn128" else (0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb,
                                         0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1)
    P = E.g1_mul(g1, a)
    Q = g2_gen(name)
    assert b == 1
    args = [H(P[0]), H(P[1]), "1", H(Q[0][0]), H(Q[0][1]), H(Q[1][0]), H(Q[1][1]), "1", "0"]
    return [int(x, 16) for x in tool("miller", ci, *args)]


# ---- the chain final exponentiation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bn128", "bls12381"])
def test_chain_constants(tool, name):
    """x and the cofactor come from the loop scalar; K is coprime to r and the chain's exponent is K times the hard part"""
    E = GO.CURVES[name]
    x_abs, h = (int(v, 16) for v in tool("x", CURVE_ID[name]))
    k = AV.CHAIN_K[name]
    assert math.gcd(k, E.R) == 1
    p, hard = E.P, (E.P ** 4 - E.P ** 2 + 1) // E.R
    if name == "bn128":
        x = x_abs
        assert 6 * x + 2 == E.loop and h == 1
        l0, l1, l2 = 12 * x ** 3 + 12 * x ** 2 + 6 * x + 1, 12 * x ** 3 + 6 * x ** 2 + 4 * x, 12 * x ** 3 + 6 * x ** 2 + 6 * x
        assert l0 + l1 * p + l2 * p ** 2 + (l1 - 1) * p ** 3 == k * hard
    else:
        x = -x_abs
        assert x_abs == E.loop and 3 * h == (x - 1) ** 2 and (p + 1 - (x + 1)) % h == 0           # #E(Fq) = p + 1 - t, t = x + 1, = h r
        assert (x - 1) ** 2 * (x + p) * (x * x + p * p - 1) + 3 == k * hard


@pytest.mark.parametrize("name", ["bn128", "bls12381"])
def test_chain_equals_final_exp_to_the_k(tool, name):
    E, ci, k = GO.CURVES[name], CURVE_ID[name], AV.CHAIN_K[name]
    rnd = random.Random("chain " + name)
    cases = [miller(tool, E, ci, name, rnd.randrange(1, E.R), 1) for _ in range(2)]
    cases.append([rnd.randrange(E.P) for _ in range(12)])                 # no Miller value: a random element
    for f in cases:
        want = E.f12_pow(f12(tool, "fexp", ci, f), k)
        assert f12(tool, "chain", ci, f) == want
        assert want != E.F12_ONE
        # on the cyclotomic subgroup (after the easy part) the Granger-Scott squaring is the squaring
        t = f12(tool, "easy", ci, f)
        assert f12(tool, "cyclo", ci, t) == f12(tool, "sqr", ci, t) == E.f12_mul(t, t)
    assert tool("isone", ci, *[H(c) for c in cases[2]]) == ["0", "0"]
    assert tool("isone", ci, *([H(1)] + ["0"] * 11)) == ["1", "1"]


@pytest.mark.parametrize("f", PV.GOLDEN_FILES + FV.GOLDEN_FILES)
def test_is_one_agrees_on_golden_pairing_inputs(tool, f):
    """the product of the Miller values of a golden proof's two pairs is one under both exponentiations; with a tampered point under neither"""
    plonk = f in PV.GOLDEN_FILES
    vk, pubs, proof = (PV if plonk else FV).golden(f)
    name = vk.get("curve", "bn128")
    E, ci = GO.CURVES[name], CURVE_ID[name]
    p, q = AV.pair_of("plonk" if plonk else "fflonk", vk, pubs, proof)
    x2, g2 = GO._g2(vk["X_2"]), g2_gen(name)
    t0, t1 = (x2, g2) if plonk else (g2, x2)
    for tamper, want in ((False, "1"), (True, "0")):
        qq = E.g1_add(q, q) if tamper else q
        m = E.f12_mul(E.miller_loop(t0, E.g1_neg(p)), E.miller_loop(t1, qq))
        assert tool("isone", ci, *[H(c) for c in m]) == [want, want]


# ---- challenges -------------------------------------------------------------------------------------------------------------------------------
def test_challenges(tool):
    seed = AV.seed_of("challenges")
    for i in (0, 1, 2, 63, 64, 4096, 2 ** 32 + 5, 2 ** 63 + 1):
        r = int(tool("challenge", 0, seed.hex(), i)[0], 16)
        assert r == AV.challenge(seed, i) and r >> 127 == 1
    assert AV.challenge(AV.seed_of("other"), 0) != AV.challenge(seed, 0)


# ---- sums and verdicts ------------------------------------------------------------------------------------------------------------------------
def _root(ci, power):
    from snarkjs_amd import zkmi
    w = np.zeros(32, np.uint8)
    zkmi.check(zkmi.lib().zkmi_fr_root(ci, int(power), zkmi.ptr(w)))
    return H(int.from_bytes(w.tobytes(), "little"))


def run_batch(tool, proto, vk, batch, seed):
    """(ok, pair_ok, codes, S_P, S_Q) of the harness for a batch [(publicSignals, proof), ...], every one with nPublic signals"""
    name = vk.get("curve", "bn128")
    E, ci = GO.CURVES[name], CURVE_ID[name]

    def g1(o):
        return [H(int(o[0]) % E.P), H(int(o[1]) % E.P), H(int(o[2] if len(o) > 2 else 1) % E.P)]
    a = [proto, ci, vk["power"], vk["nPublic"], _root(ci, vk["power"])]
    if proto == "plonk":
        a += [H(vk["k1"]), H(vk["k2"])]
        for k in ("Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3"):
            a += g1(vk[k])
    else:
        a += [H(vk[k]) for k in ("k1", "k2", "w3", "w4", "w8", "wr")] + g1(vk["C0"])
    for c in vk["X_2"]:
        a += [H(c[0]), H(c[1])]
    a += [seed.hex(), len(batch)]
    for pubs, proof in batch:
        assert len(pubs) == int(vk["nPublic"])
        if proto == "plonk":
            for k in PV.POINTS:
                a += g1(proof[k])
            a += [H(int(proof[k])) for k in PV.EVALS]
        else:
            for k in FV.POINTS:
                a += g1(proof["polynomials"][k])
            a += [H(int(proof["evaluations"][k])) for k in FV.EVALS]
        a += [H(x) for x in pubs]
    out = tool(*a)
    v = [int(x, 16) for x in out[2:6]]
    pt = lambda x, y: None if (x, y) == (0, 0) else (x, y)
    return out[0] == "1", out[1] == "1", [int(c) for c in out[6:]], pt(v[0], v[1]), pt(v[2], v[3])


def check(tool, proto, vk, batch, seed, want_ok=None):
    ok, codes, sp, sq = AV.restate(proto, vk, batch, seed)
    got = run_batch(tool, proto, vk, batch, seed)
    assert got[2] == codes
    assert got[3] == sp and got[4] == sq
    assert got[0] == ok
    if want_ok is not None:
        assert ok == want_ok
    return got


def encodings(proto, vk, pubs, proof, n):
    """the accepted proof in n encodings: itself, then one commitment in Jacobian form with a different z each"""
    out = [(pubs, proof)]
    for j in range(1, n):
        if proto == "plonk":
            E = PV.curve_of(vk)
            k = PV.POINTS[j % len(PV.POINTS)]
            out.append((pubs, PV.with_(proof, **{k: PV.jacobian(E, PV.affine(E, proof[k]), 3 + j)})))
        else:
            k = FV.POINTS[j % len(FV.POINTS)]
            out.append((pubs, FV.with_point(proof, k, FV.jacobian(FV.affine(proof["polynomials"][k]), 3 + j))))
    return out


def bad_eval(proto, vk, proof):
    """a tamper the per-proof vectors reject with code 0: one evaluation plus one"""
    if proto == "plonk":
        return PV.with_(proof, eval_a=str((int(proof["eval_a"]) + 1) % PV.curve_of(vk).R))
    return FV.with_eval(proof, "z", (int(proof["evaluations"]["z"]) + 1) % FV.E.R)


CASES = [("plonk", f) for f in PV.GOLDEN_FILES] + [("fflonk", f) for f in FV.GOLDEN_FILES]


@pytest.mark.parametrize("proto,f", CASES)
def test_sums_and_verdicts(tool, proto, f):
    vk, pubs, proof = (PV if proto == "plonk" else FV).golden(f)
    seed = AV.seed_of("sums " + f)
    good = encodings(proto, vk, pubs, proof, 4)
    ok, pair_ok, codes, sp, sq = check(tool, proto, vk, good, seed, True)
    assert codes == [1] * 4 and sp is not None and sq is not None
    assert check(tool, proto, vk, good[:1], seed, True)[0]
    # another seed: other sums, the same verdict
    other = check(tool, proto, vk, good, AV.seed_of("other " + f), True)
    assert other[3] != sp and other[4] != sq
    # one code-0 member at the first, a middle and the last position: every code is 1 and the pairing says no
    bad = (pubs, bad_eval(proto, vk, proof))
    for at in (0, 2, 3):
        batch = good[:at] + [bad] + good[at + 1:]
        got = check(tool, proto, vk, batch, seed, False)
        assert got[2] == [1] * 4 and not got[1]
    # the empty batch
    assert run_batch(tool, proto, vk, [], seed) == (True, True, [], None, None)


@pytest.mark.parametrize("proto,f", [CASES[0], CASES[2], CASES[3]])
def test_structural_failures(tool, proto, f):
    """each structural failure keeps its code at its index, stays out of the sums, and makes the batch not ok although the pairing of the rest holds"""
    mod = PV if proto == "plonk" else FV
    vk, pubs, proof = mod.golden(f)
    seed = AV.seed_of("structural " + f)
    good = encodings(proto, vk, pubs, proof, 3)
    seen = set()
    for label, pu, pr, want in mod.tampers(vk, pubs, proof, full=False):
        if want not in (-1, -2) or len(pu) != int(vk["nPublic"]):
            continue
        if label.endswith("_off_curve") and seen >= {-2} and label[0] not in "AC":
            continue
        batch = [good[0], (pu, pr), good[2]]
        got = check(tool, proto, vk, batch, seed, False)
        assert got[2] == [1, want, 1] and got[1], label
        seen.add(want)
    assert seen == {-1, -2}
    if proto == "fflonk":
        bad = FV.with_c0_off_curve(vk)
        assert check(tool, proto, bad, good[:2], seed, False)[2] == [-2, -2]


@pytest.mark.parametrize("n", FV.N_PUBLIC_CASES)
def test_sums_under_other_public_counts(tool, n):
    vk, _, proof = FV.golden(FV.GOLDEN_FILES[0])
    v, pu = FV.with_n_public(vk, n, 0x70 + n)
    got = check(tool, "fflonk", v, [(pu, proof), (pu, FV.with_point(proof, "C1", FV.jacobian(FV.affine(proof["polynomials"]["C1"]), 5)))], AV.seed_of("np %d" % n), False)
    assert got[2] == [1, 1]


# ---- host-only parts of verify_all ------------------------------------------------------------------------------------------------------------
class _Key:
    """VerifyingKey without the device: what packing and the argument checks of the aggregated calls need"""

    def __init__(self, mod, vk):
        self.curve, self.n8, self.p, self.r = mod._FQ[vk.get("curve", "bn128")]
        self.n_public = int(vk["nPublic"])
        self.handle = 1
        self.mod = mod
        self.calls = []
    record_bytes = property(lambda self: (27 * self.n8 + 192) if self.mod.__name__.endswith("plonk_verify") else (12 * self.n8 + 480))

    def pack(self, sigs, proofs):
        return self.mod.VerifyingKey.pack(self, sigs, proofs)

    def verify_all_raw(self, recs, pubs, n_sig, n, seed=None):
        self.calls.append((recs.size, pubs.size, n_sig, n, seed))
        return True, np.ones(n, np.int8)


@pytest.mark.parametrize("proto", ["plonk", "fflonk"])
def test_verify_all_packing_and_argument_checks(proto):
    from snarkjs_amd import _verify_common as vc, plonk_verify, fflonk_verify, zkmi
    mod, vec = (plonk_verify, PV) if proto == "plonk" else (fflonk_verify, FV)
    vk, pubs, proof = vec.golden(vec.GOLDEN_FILES[0])
    key = _Key(mod, vk)
    for name in ("verify_all", "verify_all_raw", "verify_many_fast"):
        assert callable(getattr(mod.VerifyingKey, name))
    seed = AV.seed_of("host")
    assert vc.verify_all(key, [pubs, pubs], [proof, proof], seed, "x") is True
    assert key.calls == [(2 * key.record_bytes, 2 * 32 * len(pubs), len(pubs), 2, seed)]
    # an out-of-range public is caught on the host: False without a device call
    assert vc.verify_all(key, [pubs, [str(key.r)] + pubs[1:]], [proof, proof], seed, "x") is False and len(key.calls) == 1
    with pytest.raises(ValueError):
        vc.verify_all(key, [pubs], [proof, proof], seed, "x")
    assert vc.new_seed(seed) == seed and len(vc.new_seed(None)) == 32 and vc.new_seed(None) != vc.new_seed(None)
    with pytest.raises(ValueError, match="32 bytes"):
        vc.new_seed(b"short")
    recs, pb, n_sig, _ = key.pack([pubs], [proof])
    with pytest.raises(ValueError, match="do not match"):
        mod.VerifyingKey.verify_all_raw(key, recs[:-1], pb, n_sig, 1, seed)
    with pytest.raises(ValueError, match="32 bytes"):
        mod.VerifyingKey.verify_all_raw(key, recs, pb, n_sig, 1, b"12")


def test_new_entry_points_fail_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    from snarkjs_amd import zkmi, plonk_verify, fflonk_verify
    L = zkmi.lib()
    buf = np.zeros(4096, np.uint8)
    ok = zkmi.C.c_int(7)
    for proto, mod, vec in (("plonk", plonk_verify, PV), ("fflonk", fflonk_verify, FV)):
        for s in ("zkmi_%s_verify_aggregate", "zkmi_%s_aggregate_trace_dev", "zkmi_%s_aggregate_phase_ms"):
            assert hasattr(L, s % proto) and s % proto in zkmi.SYMBOLS
        assert getattr(L, "zkmi_%s_verify_aggregate" % proto)(1, zkmi.ptr(buf), zkmi.ptr(buf), 2, 1, zkmi.ptr(buf), zkmi.ptr(buf), zkmi.C.byref(ok)) != 0
        assert b"no HIP device" in L.zkmi_last_error()
        assert getattr(L, "zkmi_%s_aggregate_trace_dev" % proto)(1, zkmi.ptr(buf), zkmi.ptr(buf), 2, 1, zkmi.ptr(buf), zkmi.ptr(buf), zkmi.C.byref(ok), zkmi.ptr(buf)) != 0
        assert b"no HIP device" in L.zkmi_last_error()
        vk, pubs, proof = vec.golden(vec.GOLDEN_FILES[0])
        key = _Key(mod, vk)
        recs, pb, n_sig, _ = key.pack([pubs], [proof])
        with pytest.raises(zkmi.ZkmiError, match="no HIP device"):
            mod.VerifyingKey.verify_all_raw(key, recs, pb, n_sig, 1, AV.seed_of("nodev"))


def test_addon_aggregate_entries_fail_without_device():
    node = shutil.which("node")
    addon = os.path.join(ROOT, "snarkjs_amd", "napi", "zkmi_napi.node")
    if node is None or not os.path.exists(addon):
        pytest.skip("node or the built addon is missing")
    js = ("const a=require(%r);for(const k of ['plonkVerifyAggregateAsync','fflonkVerifyAggregateAsync']) if(typeof a[k]!=='function'){console.log('missing',k);process.exit(3)}"
          "for(const f of [%r,%r]){const m=require(f);if(typeof m.VerifyingKey.prototype.verifyAll!=='function'){console.log('no verifyAll',f);process.exit(4)}}"
          "if(a.deviceCount()!==0){console.log('ok device');process.exit(0)}"
          "const z=(n)=>new Uint8Array(n);const loud=(e)=>{if(!/no HIP device|unknown verifying key/.test(e.message)){console.log(e.message);process.exit(6)}console.log('ok')};"
          "try{a.plonkVerifyAggregateAsync(1,z(1056),z(64),2,1,z(32)).then(()=>{console.log('no throw');process.exit(5)},loud)}catch(e){loud(e)}") % (
        addon, os.path.join(ROOT, "snarkjs_amd", "js", "plonk_verify_native.js"), os.path.join(ROOT, "snarkjs_amd", "js", "fflonk_verify_native.js"))
    r = subprocess.run([node, "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
