"""csrc/fflonk_verify.cuh on the CPU (tools/fflonk_verify_hosttest.hip, the same source with __device__ defined away) against the oracles:
beta gamma xi alpha y r0 r1 r2, A1 and B1 against oracle/fflonk_verify_oracle.py::verifier_values and the golden pairing_inputs, and the whole
per-proof check against tests/fflonk_verify_vectors.py::expected_code — whose own composition is checked first (it accepts the golden proofs
the reference accepted and rejects the tampers). Also the host-only parts of snarkjs_amd.fflonk_verify: packing, vk_from_zkey, refused keys.
No GPU needed; the new entry points must still refuse to run without one.

The host pairing at -O0 takes seconds per proof, so this module runs a subset of the tampers that covers every code: per golden one
point replaced / off the curve / at infinity / Jacobian (C1 and W2), ql and t2w +- 1, a + r, inv changed, every public signal case, the mixed
bad-point cases, C0 off the curve, and the nPublic = 0 / 1 / 9 / 17 keys. The other two points and the other thirteen evaluations, the mixed
batches and the wrong-count path of the device call are run by tests/test_gpu_fflonk_verify.py only."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import fflonk_verify_vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "bin", "fflonk_verify_hosttest")
SRC = os.path.join(ROOT, "tools", "fflonk_verify_hosttest.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "snarkjs_amd", "csrc")
_expected = {}


def expected(tag, vk, pubs, proof):
    """expected_code, once per distinct case of this module"""
    if tag not in _expected:
        _expected[tag] = V.expected_code(vk, pubs, proof)
    return _expected[tag]


@pytest.fixture(scope="module")
def tool():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("fflonk_verify.cuh", "kzg_verify.cuh", "pairing.cuh", "pairing_host.hpp", "curve.cuh", "field.cuh", "host_field.hpp")]
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


def run(tool, vk, pubs, proof):
    """(code, dict of the traced values) of the harness for one proof; coordinates reduced modulo q and evaluations given as they fit in 32
    bytes, as the packing of snarkjs_amd.fflonk_verify does"""
    from snarkjs_amd import zkmi
    E = V.E
    w = np.zeros(32, np.uint8)
    zkmi.check(zkmi.lib().zkmi_fr_root(0, int(vk["power"]), zkmi.ptr(w)))

    def g1(o):
        return [H(int(o[0]) % E.P), H(int(o[1]) % E.P), H(int(o[2]) % E.P)]
    a = ["verify", 0, vk["power"], len(pubs), H(int.from_bytes(w.tobytes(), "little"))] + [H(vk[k]) for k in ("k1", "k2", "w3", "w4", "w8", "wr")] + g1(vk["C0"])
    for c in vk["X_2"]:
        a += [H(c[0]), H(c[1])]
    for k in V.POINTS:
        a += g1(proof["polynomials"][k])
    a += [H(int(proof["evaluations"][k])) for k in V.EVALS] + [H(x) for x in pubs]
    out = tool(*a)
    t = [int(x, 16) for x in out[1:13]]
    val = dict(zip(("beta", "gamma", "xi", "alpha", "y", "r0", "r1", "r2"), t[:8]))
    val["A1"] = None if (t[8], t[9]) == (0, 0) else (t[8], t[9])
    val["B1"] = None if (t[10], t[11]) == (0, 0) else (t[10], t[11])
    return int(out[0]), val


def check_values(got, want):
    for k in ("beta", "gamma", "xi", "alpha", "y", "r0", "r1", "r2", "A1", "B1"):
        assert got[k] == want[k], k


def test_helper_accepts_goldens_and_rejects_tampers():
    """the yardstick itself: the composition of the two pinned oracles accepts what the reference accepted and rejects plain tampers"""
    for f in V.GOLDEN_FILES:
        vk, pubs, proof = V.golden(f)
        E = V.E
        ev = proof["evaluations"]
        assert expected(f, vk, pubs, proof) == 1
        assert V.expected_code(vk, pubs, V.with_eval(proof, "z", (int(ev["z"]) + 1) % E.R)) == 0
        assert V.expected_code(vk, pubs, V.with_eval(proof, "a", int(ev["a"]) + E.R)) == 1
        assert V.expected_code(vk, pubs, V.with_eval(proof, "inv", (int(ev["inv"]) + 1) % E.R)) == 1
        assert V.expected_code(vk, pubs, V.with_point(proof, "W1", V.obj(V.other_point(proof, "W1")))) == 0
        assert V.expected_code(vk, [str((int(pubs[0]) + 1) % E.R)] + pubs[1:], proof) == 0
        assert V.expected_code(V.with_c0_off_curve(vk), pubs, proof) == -2
        seen = set()
        for label, pu, p, want in V.tampers(vk, pubs, proof, full=False):
            if want is not None:
                assert V.expected_code(vk, pu, p) == want, label
                seen.add(want)
        assert seen == {-1, -2, -3}
    vk, pubs, proof = V.golden(V.GOLDEN_FILES[0])
    assert V.expected_code(vk, pubs, V.with_point(proof, "C1", V.jacobian(V.affine(proof["polynomials"]["C1"]), 5))) == 1


@pytest.mark.parametrize("f", V.GOLDEN_FILES)
def test_values_and_verdict_on_goldens(tool, f, golden_dir):
    vk, pubs, proof = V.golden(f)
    code, got = run(tool, vk, pubs, proof)
    check_values(got, V.values(vk, pubs, proof))
    (nx, ny), (bx, by) = json.load(open(os.path.join(golden_dir, f)))["pairing_inputs"]           # what the reference hands to pairingEq: -A1 and W2
    assert got["A1"] == (int(nx), (V.E.P - int(ny)) % V.E.P) and got["B1"] == (int(bx), int(by))
    assert code == expected(f, vk, pubs, proof) == 1


@pytest.mark.parametrize("n", V.N_PUBLIC_CASES)
def test_values_under_other_public_counts(tool, n):
    vk, _, proof = V.golden(V.GOLDEN_FILES[0])
    v, pu = V.with_n_public(vk, n, 0x70 + n)
    code, got = run(tool, v, pu, proof)
    check_values(got, V.values(v, pu, proof))
    assert code == expected(("np", n), v, pu, proof) == 0


@pytest.mark.parametrize("f", V.GOLDEN_FILES)
def test_verify_path_on_tampers(tool, f):
    vk, pubs, proof = V.golden(f)
    seen = set()
    for label, pu, p, want in V.tampers(vk, pubs, proof, full=False):
        if len(pu) != int(vk["nPublic"]):
            continue                                  # the signal count is refused before the kernel (tests of the packing and of the device)
        if want is None:
            want = expected((f, label), vk, pu, p)
        code, _ = run(tool, vk, pu, p)
        assert code == want, label
        seen.add(code)
    bad = V.with_c0_off_curve(vk)
    assert run(tool, bad, pubs, proof)[0] == expected((f, "c0"), bad, pubs, proof) == -2
    assert seen == {1, 0, -1, -2}


# ---- host-only parts of snarkjs_amd.fflonk_verify -----------------------------------------------------------------------------------------
class _Key:
    """VerifyingKey without the device call: what pack needs"""

    def __init__(self, vk):
        from snarkjs_amd import fflonk_verify as fv
        self.curve, self.n8, self.p, self.r = fv._FQ[vk["curve"]]
        self.n_public = int(vk["nPublic"])
    record_bytes = property(lambda self: 12 * self.n8 + 480)


def test_pack_forms():
    from snarkjs_amd import fflonk_verify as fv
    vk, pubs, proof = V.golden(V.GOLDEN_FILES[0])
    E = V.E
    key = _Key(vk)
    po, ev = proof["polynomials"], proof["evaluations"]
    base, pb, n_sig, pre = fv.VerifyingKey.pack(key, [pubs], [proof])
    assert key.record_bytes == 864 and base.size == 864 and pb.size == 32 * len(pubs) and n_sig == len(pubs) and pre == [None]
    word = lambda a, at, n=32: int.from_bytes(a[at:at + n].tobytes(), "little")
    for j, k in enumerate(V.POINTS):
        assert [word(base, 96 * j + 32 * c) for c in range(3)] == [int(po[k][0]), int(po[k][1]), 1], k
    for j, k in enumerate(V.EVALS):
        assert word(base, 384 + 32 * j) == int(ev[k]), k
    assert np.array_equal(fv.VerifyingKey.pack(key, [pubs], [V.with_eval(proof, "inv", 5)])[0], base)              # inv is not part of a record
    as_int = {"polynomials": {k: [int(x) for x in v] for k, v in po.items()}, "evaluations": {k: int(v) for k, v in ev.items()}}
    as_hex = {"polynomials": {k: [hex(int(x)) for x in v] for k, v in po.items()}, "evaluations": {k: hex(int(v)) for k, v in ev.items()}}
    for alt, pu in ((as_int, [int(x) for x in pubs]), (as_hex, [hex(int(x)) for x in pubs])):
        r2, p2, _, _ = fv.VerifyingKey.pack(key, [pu], [alt])
        assert np.array_equal(r2, base) and np.array_equal(p2, pb)
    jac = V.with_eval(V.with_point(V.with_point(proof, "C2", V.jacobian(V.affine(po["C2"]), 9)), "W1", ["0", "1", "0"]), "qr", int(ev["qr"]) + E.R * (1 << 20))
    r3, _, _, _ = fv.VerifyingKey.pack(key, [pubs], [jac])
    assert word(r3, 96 + 64) == 9 and not r3[192 + 64:192 + 96].any()
    assert word(r3, 384 + 32) == int(ev["qr"])                                                        # does not fit 32 bytes: reduced
    r4, _, _, _ = fv.VerifyingKey.pack(key, [pubs], [V.with_eval(proof, "a", int(ev["a"]) + E.R)])
    assert word(r4, 384 + 32 * 8) == int(ev["a"]) + E.R                                               # fits: the device reduces it
    _, _, _, pre = fv.VerifyingKey.pack(key, [[str(E.R)] + pubs[1:], pubs, [str(-1)] + pubs[1:]], [proof] * 3)
    assert pre == [-1, None, -1]
    _, p4, n_sig, _ = fv.VerifyingKey.pack(key, [pubs + ["1"]], [proof])
    assert n_sig == len(pubs) + 1 and p4.size == 32 * n_sig
    with pytest.raises(ValueError):
        fv.VerifyingKey.pack(key, [pubs, pubs[:-1]], [proof, proof])


@pytest.mark.parametrize("tag", ["fflonk_bn128_small", "fflonk_bn128_n256"])
def test_vk_from_zkey_equals_golden(tag, golden_dir):
    from snarkjs_amd import fflonk_verify as fv
    want = json.load(open(os.path.join(golden_dir, tag + ".json")))["vk"]
    got = fv.vk_from_zkey(open(os.path.join(golden_dir, tag + ".zkey"), "rb").read())
    assert list(got) == list(want)
    for k in want:
        assert got[k] == want[k], k
    with pytest.raises(ValueError, match="not fflonk"):
        fv.vk_from_zkey(open(os.path.join(golden_dir, "plonk_bn128_small.zkey"), "rb").read())


def test_rejects_other_keys():
    """refused before any device call: another protocol, BLS12-381 (the reference has no FFLONK there), an unknown curve, a vk.w that is not Fr.w[power]"""
    from snarkjs_amd import fflonk_verify as fv
    vk, _, _ = V.golden(V.GOLDEN_FILES[0])
    with pytest.raises(ValueError, match="FFLONK"):
        fv.VerifyingKey(dict(vk, protocol="plonk"))
    with pytest.raises(ValueError, match="bn128 only"):
        fv.VerifyingKey(dict(vk, curve="bls12381"))
    with pytest.raises(ValueError, match="curve"):
        fv.VerifyingKey(dict(vk, curve="bw6"))
    with pytest.raises(ValueError, match="vk.w"):
        fv.VerifyingKey(dict(vk, w=str(int(vk["w"]) + 1)))


def test_new_entry_points_fail_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    from snarkjs_amd import zkmi, fflonk_verify
    L = zkmi.lib()
    for s in ("zkmi_fflonk_vk_load", "zkmi_fflonk_verify_batch", "zkmi_fflonk_vk_release", "zkmi_fflonk_vk_info", "zkmi_fflonk_verify_trace_dev", "zkmi_fflonk_verify_last_ms"):
        assert hasattr(L, s) and s in zkmi.SYMBOLS
    vk, pubs, proof = V.golden(V.GOLDEN_FILES[0])
    with pytest.raises(zkmi.ZkmiError, match="no HIP device"):
        fflonk_verify.VerifyingKey(vk)
    with pytest.raises(zkmi.ZkmiError, match="no HIP device"):
        fflonk_verify.verify(vk, pubs, proof)
    out = np.zeros(2048, np.uint8)
    h = zkmi.C.c_uint64(0)
    assert L.zkmi_fflonk_vk_load(0, zkmi.ptr(out), zkmi.ptr(out), zkmi.ptr(out), 3, 2, zkmi.C.byref(h)) != 0
    assert b"no HIP device" in L.zkmi_last_error()
    assert L.zkmi_fflonk_verify_batch(1, zkmi.ptr(out), zkmi.ptr(out), 2, 1, zkmi.ptr(out)) != 0
    assert b"no HIP device" in L.zkmi_last_error()


def test_addon_fflonk_entries_fail_without_device():
    node = shutil.which("node")
    addon = os.path.join(ROOT, "snarkjs_amd", "napi", "zkmi_napi.node")
    if node is None or not os.path.exists(addon):
        pytest.skip("node or the built addon is missing")
    js = ("const a=require(%r);for(const k of ['fflonkVkLoad','fflonkVerifyAsync','fflonkVkRelease','fflonkVkInfo']) if(typeof a[k]!=='function'){console.log('missing',k);process.exit(3)}"
          "if(a.deviceCount()!==0){console.log('ok device');process.exit(0)}"
          "const z=(n)=>new Uint8Array(n);try{a.fflonkVkLoad(0,z(96),z(192),z(192),3,2);console.log('no throw');process.exit(4)}"
          "catch(e){if(!/no HIP device/.test(e.message)){console.log(e.message);process.exit(5)}}"
          "const {VerifyingKey}=require(%r);const vk=require(%r).vk;try{new VerifyingKey(vk);console.log('no throw js');process.exit(6)}"
          "catch(e){if(!/no HIP device/.test(e.message)){console.log(e.message);process.exit(7)}}"
          "try{new VerifyingKey(Object.assign({},vk,{curve:'bls12381'}));console.log('no throw bls');process.exit(8)}"
          "catch(e){if(!/bn128 only/.test(e.message)){console.log(e.message);process.exit(9)}}console.log('ok')") % (
        addon, os.path.join(ROOT, "snarkjs_amd", "js", "fflonk_verify_native.js"), os.path.join(ROOT, "tests", "golden", "fflonk_bn128_small.json"))
    r = subprocess.run([node, "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
