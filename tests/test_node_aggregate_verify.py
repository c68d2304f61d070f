"""The aggregated PLONK / FFLONK check from Node on the GPU: tests/js/aggregate_verify_gpu.js checks VerifyingKey.verifyAll against
VerifyingKey.verifyMany of the same key, in one process, on the golden proofs and the tampers of tests/plonk_verify_vectors.py /
tests/fflonk_verify_vectors.py. (The addon's entries failing loudly without a device: tests/test_aggregate_verify_host.py.)"""
import json
import os
import shutil
import subprocess

import pytest

import fflonk_verify_vectors as FV
import plonk_verify_vectors as PV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "snarkjs_amd", "napi", "zkmi_napi.node")
NODE = shutil.which("node")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")
def test_verify_all_matches_verify_many(tmp_path):
    sets = []
    for proto, vec in (("plonk", PV), ("fflonk", FV)):
        for f in vec.GOLDEN_FILES:
            vk, pubs, proof = vec.golden(f)
            cases = [{"label": lab, "publicSignals": pu, "proof": p} for lab, pu, p, _ in vec.tampers(vk, pubs, proof, full=False)]
            sets.append({"name": f, "protocol": proto, "vk": vk, "golden": {"publicSignals": pubs, "proof": proof}, "cases": cases})
    cf = tmp_path / "cases.json"
    cf.write_text(json.dumps(sets))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "aggregate_verify_gpu.js"), str(cf)], capture_output=True, text=True, timeout=1200, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
