"""The aggregated Groth16 check from Node on the GPU: tests/js/groth16_aggregate_verify_gpu.js checks VerifyingKey.verifyAll against
VerifyingKey.verifyMany of the same key, in one process, on 1, 65 and 130 proofs (the golden proof in distinct encodings) with and without a
tampered one, under a fixed seed and the default. (The addon's entry failing loudly without a device: tests/test_groth16_aggregate_host.py.)"""
import json
import os
import shutil
import subprocess

import pytest

import groth16_aggregate_vectors as GA
import verify_vectors as GV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "snarkjs_amd", "napi", "zkmi_napi.node")
NODE = shutil.which("node")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")
def test_verify_all_matches_verify_many(tmp_path):
    sets = []
    for f in ("groth16_bn128_n1024.json", "groth16_bls12381_n1024.json"):
        vk, pubs, proof = GV.golden(f)
        E = GA.curve_of(vk)
        proofs = [proof] + [GV.jacobian(E, proof, 2 + i, 3 + i) for i in range(1, 130)]
        sets.append({"name": f, "vk": vk, "publicSignals": pubs, "proofs": proofs, "tampered": GA.with_c_plus(E, proof, GA.alpha_of(E, vk))})
    cf = tmp_path / "cases.json"
    cf.write_text(json.dumps(sets))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "groth16_aggregate_verify_gpu.js"), str(cf)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
