"""Batch FFLONK verification from Node on the GPU: tests/js/fflonk_verify_gpu.js checks VerifyingKey.verifyMany and the
registerAll(..., {fused: true, verify: {fflonk: true}}) drop-in against the reference bundle's own fflonk.verify (staged in oracle/_ref/), in one
process, on the golden proofs and every tamper of tests/fflonk_verify_vectors.py (a + r, inv changed and the wrong count with a logger among
them) and on a key whose C0 is off the curve: return value and verdict logger messages.
(The addon's entries failing loudly without a device: tests/test_fflonk_verify_host.py.)"""
import json
import os
import shutil
import subprocess

import pytest

import fflonk_verify_vectors as V

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
    for f in V.GOLDEN_FILES:
        vk, pubs, proof = V.golden(f)
        cases = [{"label": "golden", "publicSignals": pubs, "proof": proof}]
        cases += [{"label": lab, "publicSignals": pu, "proof": p} for lab, pu, p, _ in V.tampers(vk, pubs, proof)]
        sets.append({"name": f, "vk": vk, "cases": cases})
    vk, pubs, proof = V.golden(V.GOLDEN_FILES[0])
    sets.append({"name": "C0 off the curve", "vk": V.with_c0_off_curve(vk),
                 "cases": [{"label": "golden", "publicSignals": pubs, "proof": proof}, {"label": "one_signal_more", "publicSignals": pubs + ["1"], "proof": proof}]})
    cf = tmp_path / "cases.json"
    cf.write_text(json.dumps(sets))
    r = subprocess.run([NODE] + FLAGS + [os.path.join(ROOT, "tests", "js", "fflonk_verify_gpu.js"), str(cf)], capture_output=True, text=True, timeout=1200, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
