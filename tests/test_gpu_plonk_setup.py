"""PLONK setup on the device (snarkjs_amd/plonk_setup.py, csrc/plonk_setup.cuh): setup() against the reference's keys under
tests/golden/plonk_setup_* (whole file, both curves, three circuits), and three checks that do not involve the reference, at 2^10 with a
ceremony of known trapdoor: the commitments in closed form, the permutation against a literal loop, and a proof made with the new key that
the project's own verifier accepts."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as orc
from snarkjs_amd import groth16_setup as gs
from snarkjs_amd import plonk, plonk_setup as ps, plonk_verify
from snarkjs_amd import zkmi
from snarkjs_amd.workloads import synth_r1cs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tools"))
LG = 10


def differing_sections(got, want):
    tab = gs.read_sections(gs._Source(want), b"zkey")
    return [t for t, v in sorted(tab.items()) if got[v[0][0]:v[0][0] + v[0][1]] != want[v[0][0]:v[0][0] + v[0][1]]]


@pytest.mark.parametrize("curve", ["bn128", "bls12381"])
@pytest.mark.parametrize("kind", ["edge", "mix", "tiny"])
def test_setup_equals_the_reference(curve, kind):
    r1 = os.path.join(GOLDEN, f"setup_{curve}_edge.r1cs" if kind == "edge" else f"plonk_setup_{curve}_{kind}.r1cs")
    pt = os.path.join(GOLDEN, f"setup_{curve}_p8.ptau")
    want = open(os.path.join(GOLDEN, f"plonk_setup_{curve}_{kind}.zkey"), "rb").read()
    # the edge circuit from paths (sections read by offset), the others from bytes
    zkey = ps.setup(r1, pt) if kind == "edge" else ps.setup(open(r1, "rb").read(), open(pt, "rb").read())
    if zkey != want:
        pytest.fail(f"{len(zkey)} bytes against {len(want)}; sections that differ from the reference's key: {differing_sections(zkey, want)}")


@pytest.fixture(scope="module")
def ptau_2p10(tmp_path_factory):
    """curve -> bytes of a prepared ptau whose trapdoor is known (tools/setupbench.py), made once per curve"""
    import setupbench
    made = {}

    def get(curve):
        if curve not in made:
            path = str(tmp_path_factory.mktemp("ptau") / f"{curve}.ptau")
            setupbench.trapdoor_ptau(curve, LG, path)
            made[curve] = open(path, "rb").read()
        return made[curve]
    return get


def _gen(cid, scalars):
    """k_i * G1, affine Montgomery bytes, zero for k = 0"""
    n = len(scalars)
    flat = np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in scalars), np.uint8)
    d_s, d_o = zkmi.DeviceBuffer.from_host(flat), zkmi.DeviceBuffer(n * 2 * orc.n8q(cid))
    zkmi.check(zkmi.lib().zkmi_gen_bases_from_scalars_dev(cid, 1, d_s.ptr, n, d_o.ptr))
    out = d_o.to_host().reshape(n, -1).copy()
    d_s.free(); d_o.free()
    for i, k in enumerate(scalars):
        if k == 0:
            out[i] = 0
    return out.reshape(-1)


def literal_sigma(rows, d, w, r):
    """writeSigma of src/plonk_setup.js:354-422 restated word for word on integers (k1 = 2, k2 = 3); rows = [(a, b, c)]"""
    sigma, last, first = [None] * (3 * d), {}, {}
    wi = 1

    def build(s, p):
        if s not in last:
            first[s] = p
        else:
            sigma[p] = last[s]
        last[s] = wi if p < d else (wi * 2 % r if p < 2 * d else wi * 3 % r)
    for i in range(d):
        a, b, c = rows[i] if i < len(rows) else (0, 0, 0)
        build(a, i); build(b, d + i); build(c, 2 * d + i)
        wi = wi * w % r
    for s, p in first.items():
        sigma[p] = last[s]
    return sigma


@pytest.mark.parametrize("curve", ["bn128", "bls12381"])
def test_commitments_in_closed_form_and_sigma_against_the_literal_loop(curve, ptau_2p10):
    import setupbench
    zkmi.init()
    cv = next(c for c in gs.CURVES.values() if c["name"] == curve)
    cid, r, d = cv["id"], cv["r"], 1 << LG
    r1 = synth_r1cs.write_r1cs(curve, *synth_r1cs.full_circuit(curve, n_c=140))
    zkey = ps.setup(r1, ptau_2p10(curve))
    src = gs._Source(r1)
    sr = gs.read_sections(src, b"r1cs")
    low = ps.lower(cv, gs.read_r1cs_header(src, sr), src.read(*sr[2][0]))     # the host lowering alone: no device, no P4
    z = {t: zkey[v[0][0]:v[0][0] + v[0][1]] for t, v in gs.read_sections(gs._Source(zkey), b"zkey").items()}
    o = 4 + cv["n8q"] + 4 + 32
    n_vars, n_public, dom, n_add, n_c = struct.unpack_from("<IIIII", z[2], o)
    assert dom == d and n_public == 3 and 512 < n_c <= 1024
    s1 = 2 * cv["n8q"]
    commitments = z[2][o + 20 + 64:o + 20 + 64 + 8 * s1]
    ints = lambda mont: [int.from_bytes(bytes(x), "little") for x in orc.from_mont(cid, np.frombuffer(mont, np.uint8)).reshape(-1, 32)]
    tau = setupbench.TRAPDOOR["tau"] % r
    L = ints(setupbench.lagrange_at_tau(cid, r, LG, tau).tobytes())
    w = int.from_bytes(orc.from_mont(cid, orc.fr_w(cid, LG)).tobytes(), "little")
    maps = [np.frombuffer(z[t], np.uint32).tolist() for t in (4, 5, 6)]
    sigma = literal_sigma(list(zip(*maps)), d, w, r)
    assert all(v is not None for v in sigma)
    # the 4n evaluations at stride 4 are the evaluations over the domain itself
    for col in range(3):
        ev = np.frombuffer(z[12][(col * 5 + 1) * d * 32:(col * 5 + 5) * d * 32], np.uint8).reshape(4 * d, 32)[::4]
        assert ints(ev.tobytes()) == sigma[col * d:(col + 1) * d], f"S{col + 1}"
    # the selector columns come from the host lowering (Montgomery, zero beyond the PLONK constraints), not from the device's output; sections
    # 7 - 11 must hold the same values at stride 4
    assert low["n_constraints"] == n_c and low["domain_size"] == d
    cols = [ints(low["selectors"][i * n_c * 32:(i + 1) * n_c * 32].tobytes()) + [0] * (d - n_c) for i in range(5)] + [sigma[c * d:(c + 1) * d] for c in range(3)]
    assert any(cols[0]) and any(cols[1]) and any(cols[4])
    for i in range(5):
        assert ints(np.frombuffer(z[7 + i][d * 32:], np.uint8).reshape(4 * d, 32)[::4].tobytes()) == cols[i], f"section {7 + i}"
    want = _gen(cid, [sum(x * l for x, l in zip(col, L)) % r for col in cols])
    assert commitments == want.tobytes()
    # the Lagrange section: polynomial i is 1 at w^i and 0 elsewhere on the domain
    for i in range(n_public):
        ev = np.frombuffer(z[13][(i * 5 + 1) * d * 32:(i * 5 + 5) * d * 32], np.uint8).reshape(4 * d, 32)[::4]
        assert ints(ev.tobytes()) == [1 if j == i else 0 for j in range(d)]
    ms = (zkmi.C.c_double * 4)()
    zkmi.check(zkmi.lib().zkmi_plonk_setup_phase_ms(ms))
    print(f"plonk setup {curve} 2^10 ms lowering/sigma/P4/commitments:", [round(x, 3) for x in ms])
    assert all(x > 0 for x in ms)


def _wtns(r, values):
    head = struct.pack("<I", 32) + r.to_bytes(32, "little") + struct.pack("<I", len(values))
    body = b"".join(int(v).to_bytes(32, "little") for v in values)
    return b"wtns" + struct.pack("<II", 2, 2) + struct.pack("<IQ", 1, len(head)) + head + struct.pack("<IQ", 2, len(body)) + body


@pytest.mark.parametrize("curve", ["bn128", "bls12381"])
def test_a_proof_under_the_new_key_verifies(curve, ptau_2p10):
    """setup -> plonk.prove -> VerifyingKey.verify_many on a satisfiable chain x_{i+1} = x_i^2 + b; a flipped public signal is refused"""
    cv = next(c for c in gs.CURVES.values() if c["name"] == curve)
    n_vars, n_out, n_pub, cons, wit = synth_r1cs.square_chain(curve, 1000)
    zkey = ps.setup(synth_r1cs.write_r1cs(curve, n_vars, n_out, n_pub, cons), ptau_2p10(curve))
    res = plonk.prove(zkey, _wtns(cv["r"], wit))
    assert res["publicSignals"] == [str(wit[1]), str(wit[2])]
    key = plonk_verify.VerifyingKey(plonk_verify.vk_from_zkey(zkey))
    try:
        assert key.power == LG and key.n_public == 2
        bad = [res["publicSignals"][0], str((int(res["publicSignals"][1]) + 1) % cv["r"])]
        assert key.verify_many([res["publicSignals"], bad], [res["proof"], res["proof"]]) == [True, False]
    finally:
        key.release()


NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "snarkjs_amd", "napi", "zkmi_napi.node")
BUNDLE = os.path.join(ROOT, "oracle", "_ref", "build", "snarkjs.min.js")


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")
@pytest.mark.skipif(not os.path.exists(BUNDLE), reason="reference bundle not staged in oracle/_ref")
def test_node_plonk_setup_through_the_addon():
    """registerAll(snarkjs, {plonkSetup: true}): snarkjs.plonk.setup on the BN254 edge fixture equals the golden; unregister() brings the reference back"""
    r = subprocess.run([NODE, "--harmony-optional-chaining", "--harmony-nullish", os.path.join(ROOT, "tests", "js", "plonk_setup_gpu.js")], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
