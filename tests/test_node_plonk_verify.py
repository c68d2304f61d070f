"""Batch PLONK verification from Node on the GPU: tests/js/plonk_verify_gpu.js checks VerifyingKey.verifyMany and the
registerAll(..., {fused: true, verify: {groth16: true, plonk: true}}) drop-in against the reference's own plonk.verify (bundle staged in
oracle/_ref/) on the golden proofs and the tampers of tests/plonk_verify_vectors.py, both curves: return value and logger messages.
(The addon's entries failing loudly without a device: tests/test_plonk_verify_host.py.)"""
import json
import os
import shutil
import subprocess

import pytest

import plonk_verify_vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "snarkjs_amd", "napi", "zkmi_napi.node")
NODE = shutil.which("node")
BUNDLE = os.path.join(ROOT, "oracle", "_ref", "build", "snarkjs.min.js")
FLAGS = ["--harmony-optional-chaining", "--harmony-nullish"]


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")
@pytest.mark.skipif(not os.path.exists(BUNDLE), reason="reference bundle not staged in oracle/_ref")
def test_verify_many_and_dropin_match_reference(tmp_path):
    sets = []
    for f in (V.GOLDEN_FILES[0], V.GOLDEN_FILES[2]):
        vk, pubs, proof = V.golden(f)
        cases = [{"label": "golden", "publicSignals": pubs, "proof": proof}]
        cases += [{"label": lab, "publicSignals": pu, "proof": p} for lab, pu, p, _ in V.tampers(vk, pubs, proof)]
        sets.append({"vk": vk, "cases": cases})
    cf = tmp_path / "cases.json"
    cf.write_text(json.dumps(sets))
    r = subprocess.run([NODE] + FLAGS + [os.path.join(ROOT, "tests", "js", "plonk_verify_gpu.js"), str(cf)], capture_output=True, text=True, timeout=1200, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
