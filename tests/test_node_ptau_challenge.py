"""powersOfTau.exportChallenge / challengeContribute / importResponse from Node: the addon's ptauChallengeSection and ptauImportSection, and
js/powersoftau_challenge_native.js behind registerAll(snarkjs, {ptauChallenge: true}).

 * not gpu: the addon exports the calls, refuses bad arguments and fails loudly ("no HIP device") without a device; tests/js/ptau_challenge_cpu.js holds the JS
   driver to the reference's live functions under the pinned random stream at powers 1 and 5 on both curves, with the reference's curve object in place of the
   device calls, has the reference's own powersOfTau.verify accept the file the driver imported, and shows that refused calls give the reference's outcome and
   that each hand-off case (a malformed file, a section 7 that does not serialise back, power 0, an empty entropy) reaches the saved function (bundle staged
   in oracle/_ref/).
 * gpu: tests/js/ptau_challenge_gpu.js runs the three functions unpatched and patched in one process on the power-5 files and compares bytes.
"""
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
    js = ("const a=require(%r);for(const k of ['ptauChallengeSection','ptauImportSection'])if(typeof a[k]!=='function'){console.log('missing '+k);process.exit(3)}"
          "const one=new Uint8Array(32);let m='';"
          "try{a.ptauChallengeSection(0,3,new Uint8Array(128),2,one,one,0)}catch(e){m=e.message}if(!/bad argument/.test(m)){console.log('group 3 accepted');process.exit(4)}"
          "m='';try{a.ptauChallengeSection(0,1,new Uint8Array(128),2,new Uint8Array(31),one,0)}catch(e){m=e.message}if(!/bad argument/.test(m)){console.log('short scalar accepted');process.exit(5)}"
          "m='';try{a.ptauChallengeSection(0,1,new Uint8Array(128),2,one,one,2)}catch(e){m=e.message}if(!/bad argument/.test(m)){console.log('form 2 accepted');process.exit(6)}"
          "m='';try{a.ptauImportSection(0,0,new Uint8Array(64),2)}catch(e){m=e.message}if(!/bad argument/.test(m)){console.log('group 0 accepted');process.exit(9)}"
          "if(a.deviceCount()!==0){console.log('ok device');process.exit(0)}"
          "try{a.ptauChallengeSection(0,1,new Uint8Array(128),2,one,one,0);console.log('no throw');process.exit(7)}"
          "catch(e){if(!/no HIP device/.test(e.message)){console.log(e.message);process.exit(8)}}"
          "try{a.ptauImportSection(0,1,new Uint8Array(64),2);console.log('no throw');process.exit(10)}"
          "catch(e){if(!/no HIP device/.test(e.message)){console.log(e.message);process.exit(11)}}console.log('ok')") % ADDON
    r = subprocess.run([NODE, "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


@need_node
@need_bundle
def test_the_js_driver_against_the_references_live_functions_without_a_device():
    r = subprocess.run([NODE] + FLAGS + [os.path.join(ROOT, "tests", "js", "ptau_challenge_cpu.js")], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-6000:] + r.stderr[-2000:]
    assert r.stdout.count("the reference's verify accepts the file imported here") == 4 and "FAIL" not in r.stdout
    assert r.stdout.count("handed over before any device work") == 12 and r.stdout.count("ChallengeRefusal with handOver") == 8


@pytest.mark.gpu
@need_node
@need_bundle
def test_the_three_functions_through_the_addon_match_the_reference():
    r = subprocess.run([NODE] + FLAGS + [os.path.join(ROOT, "tests", "js", "ptau_challenge_gpu.js")], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-6000:] + r.stderr[-2000:]
