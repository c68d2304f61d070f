"""The aggregated Groth16 check (csrc/groth16_aggregate.cuh) on the CPU (tools/groth16_aggregate_hosttest.hip, the same source with __device__
defined away) against tests/groth16_aggregate_vectors.py, which restates it from the pinned oracle: S_X, S_C, s and GT = final_exp(F) to the
byte, and the verdicts of F Miller(S_X, gamma) Miller(S_C, delta) M^s (accepted batches, one tamper at the first / a middle / the last
position, each structural code, points at infinity, fewer signals than nPublic, the empty batch) on both curves. Also the host-only parts of
verify_all. No GPU needed; the new entry points must still refuse to run without one.

The host pairing at -O0 takes seconds, so batches stay at or below 8 and seeds are fixed."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import groth16_aggregate_vectors as GA
import groth16_verify_oracle as GO
import verify_vectors as GV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "bin", "groth16_aggregate_hosttest")
SRC = os.path.join(ROOT, "tools", "groth16_aggregate_hosttest.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "snarkjs_amd", "csrc")
CURVE_ID = {"bn128": 0, "bls12381": 1}
FILES = ["groth16_bn128_n1024.json", "groth16_bls12381_n1024.json"]


@pytest.fixture(scope="module")
def tool():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("groth16_aggregate.cuh", "kzg_aggregate.cuh", "kzg_verify.cuh", "pairing.cuh", "pairing_host.hpp", "curve.cuh", "field.cuh",
                                                    "host_field.hpp")]
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


def run_batch(tool, vk, batch, seed):
    """(ok, pair_ok, codes, S_X, S_C, s, GT) of the harness for a batch [(publicSignals, proof), ...], every one with the same number of signals"""
    E = GA.curve_of(vk)
    ci = CURVE_ID[vk.get("curve", "bn128")]

    def g1(o):
        return [H(int(v) % E.P) for v in o[:3]]

    def g2(o):
        return [H(int(c) % E.P) for v in o[:3] for c in v]
    n_sig = len(batch[0][0]) if batch else 0
    a = ["agg", ci, len(vk["IC"]), n_sig] + g1(vk["vk_alpha_1"]) + g2(vk["vk_beta_2"]) + g2(vk["vk_gamma_2"]) + g2(vk["vk_delta_2"])
    for o in vk["IC"]:
        a += g1(o)
    a += [seed.hex(), len(batch)]
    for pubs, proof in batch:
        assert len(pubs) == n_sig
        a += g1(proof["pi_a"]) + g2(proof["pi_b"]) + g1(proof["pi_c"]) + [H(x) for x in pubs]
    out = tool(*a)
    v = [int(x, 16) for x in out[2:19]]
    pt = lambda x, y: None if (x, y) == (0, 0) else (x, y)
    return out[0] == "1", out[1] == "1", [int(c) for c in out[19:]], pt(v[0], v[1]), pt(v[2], v[3]), v[4], tuple(v[5:17])


def check(tool, vk, batch, seed, want_ok=None):
    ok, codes, sx, sc, s, gt = GA.restate(vk, batch, seed)
    got = run_batch(tool, vk, batch, seed)
    assert got[2] == codes
    assert got[3] == sx and got[4] == sc and got[5] == s
    assert got[6] == tuple(gt)
    assert got[0] == ok
    if want_ok is not None:
        assert ok == want_ok
    return got


def encodings(E, pubs, proof, n):
    """the accepted proof in n encodings: itself, then Jacobian forms with a different z each"""
    return [(pubs, proof)] + [(pubs, GV.jacobian(E, proof, 3 + j, 5 + 2 * j)) for j in range(1, n)]


def test_pow3(tool):
    """M^s is plain square-and-multiply over a 192-bit exponent: against the oracle's f12_pow, on an element outside the cyclotomic subgroup"""
    for name in ("bn128", "bls12381"):
        E = GO.CURVES[name]
        rnd = random.Random("pow3 " + name)
        f = [rnd.randrange(E.P) for _ in range(12)]
        for e in (0, 1, 2, (1 << 127) | 5, rnd.randrange(1 << 140), (1 << 192) - 1):
            assert [int(x, 16) for x in tool("pow", CURVE_ID[name], H(e), *[H(c) for c in f])] == list(E.f12_pow(f, e))


@pytest.mark.parametrize("f", FILES)
def test_sums_and_verdicts(tool, f):
    vk, pubs, proof = GV.golden(f)
    E = GA.curve_of(vk)
    seed = GA.seed_of("g16 sums " + f)
    good = encodings(E, pubs, proof, 4)
    ok, pair_ok, codes, sx, sc, s, gt = check(tool, vk, good, seed, True)
    assert codes == [1] * 4 and sx is not None and sc is not None and s >> 127 and gt != tuple(E.F12_ONE)
    assert check(tool, vk, good[:1], seed, True)[0]
    # another seed: other sums, the same verdict
    other = check(tool, vk, good, GA.seed_of("g16 other " + f), True)
    assert other[3] != sx and other[4] != sc and other[5] != s and other[6] != gt
    # one code-0 member at the first, a middle and the last position: every code is 1 and the pairing says no
    bad = (pubs, GA.with_c_plus(E, proof, GA.alpha_of(E, vk)))
    assert GV.oracle_verdict(E, vk, *bad) == 0
    for at in (0, 2, 3):
        batch = good[:at] + [bad] + good[at + 1:]
        got = check(tool, vk, batch, seed, False)
        assert got[2] == [1] * 4 and not got[1]
    # the empty batch
    assert run_batch(tool, vk, [], seed) == (True, True, [], None, None, 0, tuple(E.F12_ONE))


@pytest.mark.parametrize("f", FILES)
def test_structural_failures_and_infinity(tool, f):
    """each structural failure keeps its code at its index, contributes nothing, and makes the batch not ok although the rest holds; a proof point
    at infinity contributes what it contributes in the per-proof check"""
    vk, pubs, proof = GV.golden(f)
    E = GA.curve_of(vk)
    seed = GA.seed_of("g16 structural " + f)
    good = encodings(E, pubs, proof, 3)
    seen = set()
    for label, pu, pr, want in GV.tampers(E, vk, pubs, proof):
        if want in (-1, -2):
            got = check(tool, vk, [good[0], (pu, pr), good[2]], seed, False)
            assert got[2] == [1, want, 1] and got[1], label
            seen.add(label)
        elif label.endswith("_infinity"):
            got = check(tool, vk, [good[0], (pu, pr)], seed)
            assert got[2] == [1, 1] and got[0] == (GV.oracle_verdict(E, vk, pu, pr) == 1), label
            seen.add(label)
    assert seen >= {"public_eq_r", "a_off_curve", "b_off_curve", "pi_a_infinity", "pi_b_infinity", "pi_c_infinity"}


def test_fewer_signals_than_n_public(tool):
    vk, pubs, proof = GV.golden(FILES[0])
    assert len(pubs) >= 1
    got = check(tool, vk, [(pubs[:-1], proof), (pubs[:-1], GV.jacobian(GA.curve_of(vk), proof, 3, 5))], GA.seed_of("g16 fewer"), False)
    assert got[2] == [1, 1] and not got[1]


# ---- host-only parts of verify_all ------------------------------------------------------------------------------------------------------------
class _Key:
    """VerifyingKey without the device: what packing and the argument checks of the aggregated calls need"""

    def __init__(self, mod, vk):
        self.curve, self.n8, self.p, self.r = mod._FQ[vk.get("curve", "bn128")]
        self.n_public = len(vk["IC"]) - 1
        self.handle = 1
        self.mod = mod
        self.calls = []
    record_bytes = property(lambda self: 12 * self.n8)

    def pack(self, sigs, proofs):
        return self.mod.VerifyingKey.pack(self, sigs, proofs)

    def verify_all_raw(self, recs, pubs, n_sig, n, seed=None):
        self.calls.append((recs.size, pubs.size, n_sig, n, seed))
        return True, np.ones(n, np.int8)


def test_verify_all_packing_and_argument_checks():
    from snarkjs_amd import _verify_common as vc, groth16_verify
    vk, pubs, proof = GV.golden(FILES[0])
    key = _Key(groth16_verify, vk)
    for name in ("verify_all", "verify_all_raw", "verify_many_fast", "aggregate_trace"):
        assert callable(getattr(groth16_verify.VerifyingKey, name))
    seed = GA.seed_of("host")
    assert vc.verify_all(key, [pubs, pubs], [proof, proof], seed, None) is True
    assert key.calls == [(2 * key.record_bytes, 2 * 32 * len(pubs), len(pubs), 2, seed)]
    # fewer signals than nPublic go to the device; more are refused while packing, as in verify_codes
    assert vc.verify_all(key, [pubs[:-1]], [proof], seed, None) is True and key.calls[-1][2] == len(pubs) - 1
    with pytest.raises(ValueError, match="nPublic"):
        vc.verify_all(key, [pubs + ["1"]], [proof], seed, None)
    # an out-of-range public is caught on the host: False without a device call
    assert vc.verify_all(key, [pubs, [str(key.r)] + pubs[1:]], [proof, proof], seed, None) is False and len(key.calls) == 2
    recs, pb, n_sig, _ = key.pack([pubs], [proof])
    with pytest.raises(ValueError, match="do not match"):
        groth16_verify.VerifyingKey.verify_all_raw(key, recs[:-1], pb, n_sig, 1, seed)
    with pytest.raises(ValueError, match="32 bytes"):
        groth16_verify.VerifyingKey.verify_all_raw(key, recs, pb, n_sig, 1, b"12")


def test_new_entry_points_fail_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    from snarkjs_amd import zkmi, groth16_verify
    L = zkmi.lib()
    buf = np.zeros(4096, np.uint8)
    ok = zkmi.C.c_int(7)
    for s in ("zkmi_groth16_verify_aggregate", "zkmi_groth16_aggregate_trace_dev", "zkmi_groth16_aggregate_phase_ms"):
        assert hasattr(L, s) and s in zkmi.SYMBOLS
    assert L.zkmi_groth16_verify_aggregate(1, zkmi.ptr(buf), zkmi.ptr(buf), 2, 1, zkmi.ptr(buf), zkmi.ptr(buf), zkmi.C.byref(ok)) != 0
    assert b"no HIP device" in L.zkmi_last_error()
    assert L.zkmi_groth16_aggregate_trace_dev(1, zkmi.ptr(buf), zkmi.ptr(buf), 2, 1, zkmi.ptr(buf), zkmi.ptr(buf), zkmi.C.byref(ok), zkmi.ptr(buf)) != 0
    assert b"no HIP device" in L.zkmi_last_error()
    vk, pubs, proof = GV.golden(FILES[0])
    key = _Key(groth16_verify, vk)
    recs, pb, n_sig, _ = key.pack([pubs], [proof])
    with pytest.raises(zkmi.ZkmiError, match="no HIP device"):
        groth16_verify.VerifyingKey.verify_all_raw(key, recs, pb, n_sig, 1, GA.seed_of("nodev"))


def test_addon_aggregate_entry_fails_without_device():
    node = shutil.which("node")
    addon = os.path.join(ROOT, "snarkjs_amd", "napi", "zkmi_napi.node")
    if node is None or not os.path.exists(addon):
        pytest.skip("node or the built addon is missing")
    js = ("const a=require(%r);if(typeof a.groth16VerifyAggregateAsync!=='function'){console.log('missing');process.exit(3)}"
          "const m=require(%r);if(typeof m.VerifyingKey.prototype.verifyAll!=='function'){console.log('no verifyAll');process.exit(4)}"
          "if(a.deviceCount()!==0){console.log('ok device');process.exit(0)}"
          "const z=(n)=>new Uint8Array(n);const loud=(e)=>{if(!/no HIP device|unknown verifying key/.test(e.message)){console.log(e.message);process.exit(6)}console.log('ok')};"
          "try{a.groth16VerifyAggregateAsync(1,z(384),z(64),2,1,z(32)).then(()=>{console.log('no throw');process.exit(5)},loud)}catch(e){loud(e)}") % (
        addon, os.path.join(ROOT, "snarkjs_amd", "js", "groth16_verify_native.js"))
    r = subprocess.run([node, "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
