"""Batch Groth16 verification from Node: the addon's groth16VkLoad / groth16VerifyAsync / groth16VkRelease and js/groth16_verify_native.js.

 * not gpu: the addon exports the three entries and they fail loudly ("no HIP device") without a device.
 * gpu: tests/js/verify_gpu.js checks verifyMany and the registerAll(..., {fused: true, verify: true}) drop-in against the reference's own
   groth16.verify (bundle staged in oracle/_ref/) on valid, tampered, Jacobian-form, off-subgroup and pi_a / pi_c-at-infinity proofs.
"""
import json
import os
import shutil
import subprocess

import pytest

import groth16_verify_oracle as O
import verify_vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "snarkjs_amd", "napi", "zkmi_napi.node")
NODE = shutil.which("node")
BUNDLE = os.path.join(ROOT, "oracle", "_ref", "build", "snarkjs.min.js")
need_node = pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")
FLAGS = ["--harmony-optional-chaining", "--harmony-nullish"]


@need_node
def test_addon_verify_entries_fail_without_device():
    js = ("const a=require(%r);for(const k of ['groth16VkLoad','groth16VerifyAsync','groth16VkRelease']) if(typeof a[k]!=='function'){console.log('missing',k);process.exit(3)}"
          "if(a.deviceCount()!==0){console.log('ok device');process.exit(0)}"
          "const z=(n)=>new Uint8Array(n);try{a.groth16VkLoad(0,z(96),z(192),z(192),z(192),z(96),0);console.log('no throw');process.exit(4)}"
          "catch(e){if(!/no HIP device/.test(e.message)){console.log(e.message);process.exit(5)}}"
          "const {VerifyingKey}=require(%r);const vk=require(%r).vk;try{new VerifyingKey(vk);console.log('no throw js');process.exit(6)}"
          "catch(e){if(!/no HIP device/.test(e.message)){console.log(e.message);process.exit(7)}}console.log('ok')") % (
        ADDON, os.path.join(ROOT, "snarkjs_amd", "js", "groth16_verify_native.js"), os.path.join(ROOT, "tests", "golden", "groth16_bn128_n1024.json"))
    r = subprocess.run([NODE, "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@need_node
@pytest.mark.skipif(not os.path.exists(BUNDLE), reason="reference bundle not staged in oracle/_ref")
def test_verify_many_and_dropin_match_reference(tmp_path):
    sets = []
    for f in ("groth16_bn128_n1024.json", "groth16_bls12381_n1024.json"):
        vk, pubs, proof = V.golden(f)
        E = O.BN254 if vk["curve"] == "bn128" else O.BLS12381
        cases = [{"label": "golden", "publicSignals": pubs, "proof": proof}]
        # pi_b at infinity follows the oracle (the pair contributes 1; tests/test_gpu_verify.py): the reference's BLS12-381 pairingEq accepts the golden
        # proof with pi_b = infinity, which no pairing product can justify, so that case is not compared with the bundle here
        cases += [{"label": lab, "publicSignals": pu, "proof": p} for lab, pu, p, _ in V.tampers(E, vk, pubs, proof) if lab != "pi_b_infinity"]
        sets.append({"vk": vk, "cases": cases})
    cf = tmp_path / "cases.json"
    cf.write_text(json.dumps(sets))
    r = subprocess.run([NODE] + FLAGS + [os.path.join(ROOT, "tests", "js", "verify_gpu.js"), str(cf)], capture_output=True, text=True, timeout=1200, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
