"""Groth16 phase 2 from Node: the addon's groupScale and js/groth16_phase2_native.js behind registerAll(snarkjs, {phase2: true}).

 * not gpu: the addon exports groupScale, which fails loudly ("no HIP device") without a device; the host entry points of the contribution answer through
   the checked call table without one.
 * gpu: tests/js/phase2_gpu.js runs contribute -> beacon -> contribute unpatched and patched in one process and compares keys and hashes; the reference's
   own verifiers judge the device-made key (bundle staged in oracle/_ref/).
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "snarkjs_amd", "napi", "zkmi_napi.node")
NODE = shutil.which("node")
BUNDLE = os.path.join(ROOT, "oracle", "_ref", "build", "snarkjs.min.js")
need_node = pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")
FLAGS = ["--harmony-optional-chaining", "--harmony-nullish"]


@need_node
def test_addon_entries_without_a_device():
    v = json.load(open(os.path.join(ROOT, "tests", "golden", "phase2_golden.json")))["vectors"]["bn128"]
    js = ("const a=require(%r);if(typeof a.groupScale!=='function'){console.log('missing groupScale');process.exit(3)}"
          "const v=%s,prv=new Uint8Array(32),s=new Uint8Array(64),sx=new Uint8Array(64),g2=new Uint8Array(128);"
          "a.call('zkmi_phase2_key_from_seed',0,new Uint32Array(v.f.seed),prv,s,sx);"
          "if(Buffer.from(prv).toString('hex')!==v.f.fr||Buffer.from(s).toString('hex')!==v.f.g1){console.log('key_from_seed differs');process.exit(4)}"
          "a.call('zkmi_phase2_hash_to_g2',0,new Uint8Array(Buffer.from(v.h.transcript,'hex')),g2);"
          "if(Buffer.from(g2).toString('hex')!==v.h.g2){console.log('hash_to_g2 differs');process.exit(5)}"
          "if(a.deviceCount()!==0){console.log('ok device');process.exit(0)}"
          "try{a.groupScale(0,1,new Uint8Array(64),new Uint8Array(64),1,new Uint8Array(32));console.log('no throw');process.exit(6)}"
          "catch(e){if(!/no HIP device/.test(e.message)){console.log(e.message);process.exit(7)}}console.log('ok')") % (
        ADDON, json.dumps({"f": v["fromRng"][0], "h": v["hashToG2"][0]}))
    r = subprocess.run([NODE, "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@need_node
@pytest.mark.skipif(not os.path.exists(BUNDLE), reason="reference bundle not staged in oracle/_ref")
def test_contribute_and_beacon_through_the_addon_match_the_reference():
    r = subprocess.run([NODE] + FLAGS + [os.path.join(ROOT, "tests", "js", "phase2_gpu.js")], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
