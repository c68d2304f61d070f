"""Groth16 setup on the device (snarkjs_amd/groth16_setup.py, csrc/groth16_setup.cuh): new_zkey against the reference's keys under
tests/golden/setup_* (whole file and csHash, both curves, the edge and the full circuit), and a closed form that does not involve the
reference: with a known trapdoor every section is (a sum of coefficients times L_c(tau)) * G."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as orc
from snarkjs_amd import groth16_setup as gs
from snarkjs_amd import zkmi
from snarkjs_amd.workloads import synth_r1cs
from synth_valid_groth16 import TRAPDOOR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("curve", ["bn128", "bls12381"])
@pytest.mark.parametrize("kind", ["edge", "full"])
def test_new_zkey_equals_the_reference(curve, kind):
    r1, pt = os.path.join(GOLDEN, f"setup_{curve}_{kind}.r1cs"), os.path.join(GOLDEN, f"setup_{curve}_p8.ptau")
    want = open(os.path.join(GOLDEN, f"setup_{curve}_{kind}.zkey"), "rb").read()
    # the edge circuit from paths (sections read by offset), the full one from bytes
    zkey, cs_hash = gs.new_zkey(r1, pt) if kind == "edge" else gs.new_zkey(open(r1, "rb").read(), open(pt, "rb").read())
    assert cs_hash.hex() == json.load(open(os.path.join(GOLDEN, "setup_golden.json")))[f"setup_{curve}_{kind}.zkey"]["csHash"]
    if zkey != want:
        src = gs._Source(want)
        tab = gs.read_sections(src, b"zkey")
        bad = [t for t, v in sorted(tab.items()) if zkey[v[0][0]:v[0][0] + v[0][1]] != want[v[0][0]:v[0][0] + v[0][1]]]
        pytest.fail(f"sections that differ from the reference's key: {bad}")


def _gen(cid, group, scalars):
    """k_i * G, affine Montgomery bytes (zkmi_gen_bases_from_scalars_dev), zero for k = 0"""
    n = len(scalars)
    flat = np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in scalars), np.uint8)
    d_s, d_o = zkmi.DeviceBuffer.from_host(flat), zkmi.DeviceBuffer(n * 2 * group * orc.n8q(cid))
    zkmi.check(zkmi.lib().zkmi_gen_bases_from_scalars_dev(cid, group, d_s.ptr, n, d_o.ptr))
    out = d_o.to_host().reshape(n, -1).copy()
    d_s.free(); d_o.free()
    for i, k in enumerate(scalars):
        if k == 0:
            out[i] = 0
    return out.reshape(-1)


@pytest.mark.parametrize("curve", ["bn128", "bls12381"])
def test_closed_form_at_2p10(curve):
    zkmi.init()
    cv = next(c for c in gs.CURVES.values() if c["name"] == curve)
    cid, r = cv["id"], cv["r"]
    lg, n_c, n_vars, n_public = 10, 1000, 300, 3
    d = 1 << lg
    tau, alpha, beta = (TRAPDOOR[k] % r for k in ("tau", "alpha", "beta"))
    w = int.from_bytes(orc.from_mont(cid, orc.fr_w(cid, lg)).tobytes(), "little")
    zn = (pow(tau, d, r) - 1) * pow(d, -1, r) % r
    L = [pow(w, c, r) * zn % r * pow((tau - pow(w, c, r)) % r, -1, r) % r for c in range(d)]     # L_c(tau) = w^c (tau^n - 1) / (n (tau - w^c))
    nv, n_out, n_pub_in, cons = synth_r1cs.one_signal_circuit(curve, n_c, n_vars, n_public, seed=0xc105ed)
    r1 = synth_r1cs.write_r1cs(curve, nv, n_out, n_pub_in, cons)
    src = gs._Source(r1)
    sr = gs.read_sections(src, b"r1cs")
    hdr = gs.read_r1cs_header(src, sr)
    assert gs.circuit_power(hdr) == lg and hdr["nOutputs"] + hdr["nPubInputs"] == n_public
    n_h = gs.hashed_h_points(d)
    dev = gs.device_sections(cv, hdr, d, n_h, src.read(*sr[2][0]), _gen(cid, 1, L), _gen(cid, 2, L), _gen(cid, 1, [alpha * x % r for x in L]),
                             _gen(cid, 1, [beta * x % r for x in L]), _gen(cid, 1, [pow(tau, i, r) for i in range(d + n_h)]))
    u, v, ww = [0] * n_vars, [0] * n_vars, [0] * n_vars
    for c, (a, b, cc) in enumerate(cons):
        for s, k in a:
            u[s] = (u[s] + k * L[c]) % r
        for s, k in b:
            v[s] = (v[s] + k * L[c]) % r
        for s, k in cc:
            ww[s] = (ww[s] + k * L[c]) % r
    for s in range(n_public + 1):
        u[s] = (u[s] + L[n_c + s]) % r
    icc = [(beta * u[s] + alpha * v[s] + ww[s]) % r for s in range(n_vars)]
    s1 = 2 * cv["n8q"]
    assert dev["a"].tobytes() == _gen(cid, 1, u).tobytes()
    assert dev["b1"].tobytes() == _gen(cid, 1, v).tobytes()
    assert dev["b2"].tobytes() == _gen(cid, 2, v).tobytes()
    both = _gen(cid, 1, icc).tobytes()
    assert dev["ic"].tobytes() == both[:(n_public + 1) * s1] and dev["c"].tobytes() == both[(n_public + 1) * s1:]
    h = _gen(cid, 1, [(pow(tau, i + d, r) - pow(tau, i, r)) % r for i in range(n_h)])
    assert dev["h"].tobytes() == orc.group_convert(cid, 1, "LEMtoU", h).tobytes()
    ms = (zkmi.C.c_double * 5)()
    zkmi.check(zkmi.lib().zkmi_groth16_setup_phase_ms(ms))
    print(f"setup {curve} 2^10 kernel ms A/B1/B2/ICC/H:", [round(x, 3) for x in ms])
    assert all(x > 0 for x in ms)


NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "snarkjs_amd", "napi", "zkmi_napi.node")
BUNDLE = os.path.join(ROOT, "oracle", "_ref", "build", "snarkjs.min.js")


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")
@pytest.mark.skipif(not os.path.exists(BUNDLE), reason="reference bundle not staged in oracle/_ref")
def test_node_new_zkey_through_the_addon():
    """registerAll(snarkjs, {setup: true}): snarkjs.zKey.newZKey on the BN254 edge fixture equals the golden; unregister() brings the reference back"""
    r = subprocess.run([NODE, "--harmony-optional-chaining", "--harmony-nullish", os.path.join(ROOT, "tests", "js", "setup_gpu.js")], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
