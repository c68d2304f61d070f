"""zKey.verifyFromInit / verifyFromR1cs from Node: the addon's sameRatioBatch, phase2SectionRatio and phase2HRatio and js/groth16_phase2_verify_native.js behind
registerAll(snarkjs, {phase2Verify: true}).

 * not gpu: the addon exports the three calls, which fail loudly ("no HIP device") without a device, and the generator's host entry points answer through the
   checked call table; tests/js/phase2_verify_cpu.js holds the JS driver's parsing, order and lines to the reference's own verifyFromInit with the reference's
   curve object in place of the device calls (bundle staged in oracle/_ref/).
 * gpu: tests/js/phase2_verify_gpu.js runs both functions unpatched and patched in one process and compares verdicts and lines.
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
need_bundle = pytest.mark.skipif(not os.path.exists(BUNDLE), reason="reference bundle not staged in oracle/_ref")
FLAGS = ["--harmony-optional-chaining", "--harmony-nullish"]


@need_node
def test_addon_entries_without_a_device():
    v = json.load(open(os.path.join(ROOT, "tests", "golden", "phase2_golden.json")))["vectors"]["bn128"]["fromRng"][0]
    js = ("const a=require(%r);for(const f of ['sameRatioBatch','phase2SectionRatio','phase2HRatio'])if(typeof a[f]!=='function'){console.log('missing '+f);process.exit(3)}"
          "const v=%s,seed=new Uint32Array(v.seed),fr=new Uint8Array(32),w=new Uint8Array(8),ks=new Uint8Array(64),ks2=new Uint8Array(32);"
          "a.call('zkmi_chacha_fr_host',0,seed,fr,1,w);"
          "if(Buffer.from(fr).toString('hex')!==v.fr||new DataView(w.buffer).getUint32(0,true)!==2*v.frDraws){console.log('chacha_fr_host differs');process.exit(4)}"
          "a.call('zkmi_chacha_struct_words_host',seed,0,ks,16);a.call('zkmi_chacha_struct_words_host',seed,5,ks2,8);"
          "if(Buffer.compare(Buffer.from(ks.subarray(20,52)),Buffer.from(ks2))!==0){console.log('keystream by position differs');process.exit(5)}"
          "let m='';try{a.call('zkmi_chacha_struct_words_host',seed,0,new Uint8Array(60),16)}catch(e){m=e.message}"
          "if(!/shorter/.test(m)){console.log('short buffer accepted');process.exit(8)}"
          "m='';try{a.sameRatioBatch(0,new Uint8Array(64),new Uint8Array(64),new Uint8Array(128),new Uint8Array(127),1)}catch(e){m=e.message}"
          "if(!/bad argument/.test(m)){console.log('short point buffer accepted');process.exit(9)}"
          "if(a.deviceCount()!==0){console.log('ok device');process.exit(0)}"
          "for(const f of [()=>a.sameRatioBatch(0,new Uint8Array(64),new Uint8Array(64),new Uint8Array(128),new Uint8Array(128),1),"
          "()=>a.phase2SectionRatio(0,new Uint8Array(64),new Uint8Array(64),1,new Uint8Array(32)),()=>a.phase2HRatio(0,new Uint8Array(192),new Uint8Array(128),1,new Uint8Array(32))])"
          "{try{f();console.log('no throw');process.exit(6)}catch(e){if(!/no HIP device/.test(e.message)){console.log(e.message);process.exit(7)}}}console.log('ok')") % (
        ADDON, json.dumps(v))
    r = subprocess.run([NODE, "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


@need_node
@need_bundle
def test_the_js_driver_against_the_references_verify_without_a_device():
    r = subprocess.run([NODE] + FLAGS + [os.path.join(ROOT, "tests", "js", "phase2_verify_cpu.js")], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-6000:] + r.stderr[-2000:]


@pytest.mark.gpu
@need_node
@need_bundle
def test_verify_from_init_and_from_r1cs_through_the_addon_match_the_reference():
    r = subprocess.run([NODE] + FLAGS + [os.path.join(ROOT, "tests", "js", "phase2_verify_gpu.js")], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-6000:] + r.stderr[-2000:]
