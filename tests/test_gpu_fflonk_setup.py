"""FFLONK setup on the device (snarkjs_amd/fflonk_setup.py, csrc/fflonk_setup.cuh): setup() against the reference's keys under
tests/golden/fflonk_setup_* (whole file, five circuits, domains 8 to 256), and checks that do not involve the reference, at 2^10 with a ceremony of
known trapdoor: the C0 commitment in closed form, the permutation against a literal loop, and a proof made with the new key that the project's own
verifier accepts.

The golden domains are the smallest at which each kernel meets its cases: 8 and 16 are less than a wave; 32 (rows30) has the last-two-rows rule
without a signal-0 filler row, the others with; 256 is more than one block of 256 threads for the sigma gather (768 positions) and the C0 kernel
(2 048 elements)."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as orc
from snarkjs_amd import fflonk, fflonk_setup as fs, fflonk_verify
from snarkjs_amd import groth16_setup as gs
from snarkjs_amd import zkmi
from snarkjs_amd.workloads import synth_r1cs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tools"))
LG = 10
P8, P12S = "setup_bn128_p8.ptau", "fflonk_setup_bn128_p12s.ptau"
FIXTURES = {"tiny": ("plonk_setup_bn128_tiny.r1cs", P8), "quirks": ("fflonk_setup_bn128_quirks.r1cs", P8), "rows30": ("fflonk_setup_bn128_rows30.r1cs", P8),
            "mix": ("plonk_setup_bn128_mix.r1cs", P12S), "edge": ("setup_bn128_edge.r1cs", P12S)}
BN = next(c for c in gs.CURVES.values() if c["name"] == "bn128")
R = BN["r"]


def differing_sections(got, want):
    tab = gs.read_sections(gs._Source(want), b"zkey")
    return [t for t, v in sorted(tab.items()) if got[v[0][0]:v[0][0] + v[0][1]] != want[v[0][0]:v[0][0] + v[0][1]]]


@pytest.mark.parametrize("kind", list(FIXTURES))
def test_setup_equals_the_reference(kind):
    r1, pt = (os.path.join(GOLDEN, f) for f in FIXTURES[kind])
    want = open(os.path.join(GOLDEN, f"fflonk_setup_bn128_{kind}.zkey"), "rb").read()
    # the edge circuit from paths (sections read by offset), the others from bytes
    zkey = fs.setup(r1, pt) if kind == "edge" else fs.setup(open(r1, "rb").read(), open(pt, "rb").read())
    if zkey != want:
        pytest.fail(f"{len(zkey)} bytes against {len(want)}; sections that differ from the reference's key: {differing_sections(zkey, want)}")


@pytest.fixture(scope="module")
def ptau_2p10(tmp_path_factory):
    """bytes of a ptau whose trapdoor is known and whose first 9 * 2^10 + 18 tauG1 powers are real (tools/setupbench.py), made once"""
    import setupbench
    zkmi.init()
    path = str(tmp_path_factory.mktemp("ptau") / "fflonk.ptau")
    setupbench.fflonk_trapdoor_ptau(LG, path)
    return open(path, "rb").read()


def _gen(scalars):
    """k_i * G1, affine Montgomery bytes, zero for k = 0"""
    n = len(scalars)
    flat = np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in scalars), np.uint8)
    d_s, d_o = zkmi.DeviceBuffer.from_host(flat), zkmi.DeviceBuffer(n * 64)
    zkmi.check(zkmi.lib().zkmi_gen_bases_from_scalars_dev(0, 1, d_s.ptr, n, d_o.ptr))
    out = d_o.to_host().reshape(n, -1).copy()
    d_s.free(); d_o.free()
    for i, k in enumerate(scalars):
        if k == 0:
            out[i] = 0
    return out.reshape(-1)


def literal_sigma(rows, d, w, r):
    """writeSigma of src/fflonk_setup.js:340-415 restated word for word on integers (k1 = 2, k2 = 3); rows = [(a, b, c)]"""
    sigma, last, first = [None] * (3 * d), {}, {}
    wi = 1

    def build(s, p):
        if s not in last:
            first[s] = p
        else:
            sigma[p] = last[s]
        last[s] = wi if p < d else (wi * 2 % r if p < 2 * d else wi * 3 % r)
    for i in range(d):
        if i < len(rows):
            a, b, c = rows[i]
            build(a, i); build(b, d + i); build(c, 2 * d + i)
        elif i < d - 2:
            build(0, i); build(0, d + i); build(0, 2 * d + i)
        else:
            sigma[i], sigma[d + i], sigma[2 * d + i] = wi, wi * 2 % r, wi * 3 % r
        wi = wi * w % r
    for s, p in first.items():
        sigma[p] = last[s]
    return sigma


def test_c0_in_closed_form_and_sigma_against_the_literal_loop(ptau_2p10):
    import setupbench
    d = 1 << LG
    r1 = synth_r1cs.write_r1cs("bn128", *synth_r1cs.full_circuit("bn128", n_c=120))
    zkey = fs.setup(r1, ptau_2p10)
    src = gs._Source(r1)
    sr = gs.read_sections(src, b"r1cs")
    low = fs.lower(BN, gs.read_r1cs_header(src, sr), src.read(*sr[2][0]))     # the host lowering alone: no device
    z = {t: zkey[v[0][0]:v[0][0] + v[0][1]] for t, v in gs.read_sections(gs._Source(zkey), b"zkey").items()}
    o = 4 + 32 + 4 + 32
    _n_vars, n_public, dom, _n_add, n_c = struct.unpack_from("<IIIII", z[2], o)
    assert dom == d and n_public == 3 and 256 < n_c <= d - 2
    assert low["n_constraints"] == n_c and low["domain_size"] == d
    commitment = z[2][-64:]
    ints = lambda mont: [int.from_bytes(bytes(x), "little") for x in orc.from_mont(0, np.frombuffer(mont, np.uint8)).reshape(-1, 32)]
    w = int.from_bytes(orc.from_mont(0, orc.fr_w(0, LG)).tobytes(), "little")
    maps = [np.frombuffer(z[t], np.uint32).tolist() for t in (4, 5, 6)]
    sigma = literal_sigma(list(zip(*maps)), d, w, R)
    assert all(v is not None for v in sigma)
    # each block of 4n evaluations at stride 4 is its column: the selectors of the host lowering (zero beyond the rows), sigma of the literal loop
    cols = [ints(low["selectors"][i * n_c * 32:(i + 1) * n_c * 32].tobytes()) + [0] * (d - n_c) for i in range(5)] + [sigma[c * d:(c + 1) * d] for c in range(3)]
    assert all(any(c) for c in cols[:5]), "every selector column holds something"
    for i in range(8):
        assert len(z[7 + i]) == 5 * d * 32
        assert ints(np.frombuffer(z[7 + i][d * 32:], np.uint8).reshape(4 * d, 32)[::4].tobytes()) == cols[i], f"section {7 + i}"
    # section 17 and its commitment, from the key's own coefficient sections, on integers
    coefs = [ints(z[sec][:d * 32]) for sec in (7, 8, 10, 9, 11, 12, 13, 14)]
    c0 = [coefs[t % 8][t // 8] for t in range(8 * d)]
    assert ints(z[17]) == c0 and len(z[17]) == 8 * d * 32
    tau = setupbench.TRAPDOOR["tau"] % R
    acc = 0
    for c in reversed(c0):
        acc = (acc * tau + c) % R
    assert acc != 0 and commitment == _gen([acc]).tobytes()
    # the Lagrange section: polynomial i is 1 at w^i and 0 elsewhere on the domain
    assert len(z[15]) == n_public * 5 * d * 32
    for i in range(n_public):
        ev = np.frombuffer(z[15][(i * 5 + 1) * d * 32:(i * 5 + 5) * d * 32], np.uint8).reshape(4 * d, 32)[::4]
        assert ints(ev.tobytes()) == [1 if j == i else 0 for j in range(d)]
    ms = (zkmi.C.c_double * 4)()
    zkmi.check(zkmi.lib().zkmi_fflonk_setup_phase_ms(ms))
    print("fflonk setup 2^10 ms lowering/sigma/P4/C0+commitment:", [round(x, 3) for x in ms])
    assert all(x > 0 for x in ms)


def _wtns(r, values):
    head = struct.pack("<I", 32) + r.to_bytes(32, "little") + struct.pack("<I", len(values))
    body = b"".join(int(v).to_bytes(32, "little") for v in values)
    return b"wtns" + struct.pack("<II", 2, 2) + struct.pack("<IQ", 1, len(head)) + head + struct.pack("<IQ", 2, len(body)) + body


def test_a_proof_under_the_new_key_verifies(ptau_2p10):
    """setup -> fflonk.prove -> VerifyingKey.verify_many on a satisfiable chain x_{i+1} = x_i^2 + b; a flipped public signal is refused"""
    n_vars, n_out, n_pub, cons, wit = synth_r1cs.square_chain("bn128", 1000)
    zkey = fs.setup(synth_r1cs.write_r1cs("bn128", n_vars, n_out, n_pub, cons), ptau_2p10)
    res = fflonk.prove(zkey, _wtns(R, wit))
    assert res["publicSignals"] == [str(wit[1]), str(wit[2])]
    key = fflonk_verify.VerifyingKey(fflonk_verify.vk_from_zkey(zkey))
    try:
        assert key.power == LG and key.n_public == 2
        bad = [res["publicSignals"][0], str((int(res["publicSignals"][1]) + 1) % R)]
        assert key.verify_many([res["publicSignals"], bad], [res["proof"], res["proof"]]) == [True, False]
    finally:
        key.release()


NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "snarkjs_amd", "napi", "zkmi_napi.node")
BUNDLE = os.path.join(ROOT, "oracle", "_ref", "build", "snarkjs.min.js")


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")
@pytest.mark.skipif(not os.path.exists(BUNDLE), reason="reference bundle not staged in oracle/_ref")
def test_node_fflonk_setup_through_the_addon():
    """registerAll(snarkjs, {fflonkSetup: true}): snarkjs.fflonk.setup on the edge fixture equals the golden; unregister() brings the reference back; a
    BLS12-381 ceremony reaches the original function"""
    r = subprocess.run([NODE, "--harmony-optional-chaining", "--harmony-nullish", os.path.join(ROOT, "tests", "js", "fflonk_setup_gpu.js")], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
