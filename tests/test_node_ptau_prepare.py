"""powersOfTau.preparePhase2 / convert from Node: the addon's ptauLagrangeSection and js/powersoftau_prepare_native.js behind registerAll(snarkjs, {ptauPrepare: true}).

 * not gpu: the addon exports the call, refuses bad arguments and fails loudly ("no HIP device") without a device; tests/js/ptau_prepare_cpu.js holds the JS
   driver's parsing and bytes to the reference's live preparePhase2 / convert on the committed files, with the reference's curve object in place of the device
   call, and shows that files that are not well-formed reach the saved function (bundle staged in oracle/_ref/).
 * gpu: tests/js/ptau_prepare_gpu.js runs both functions unpatched and patched in one process and compares bytes.
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
def test_addon_entry_without_a_device():
    js = ("const a=require(%r);if(typeof a.ptauLagrangeSection!=='function'){console.log('missing ptauLagrangeSection');process.exit(3)}"
          "let m='';try{a.ptauLagrangeSection(0,3,new Uint8Array(128),2,0,1,0)}catch(e){m=e.message}if(!/bad argument/.test(m)){console.log('group 3 accepted');process.exit(4)}"
          "m='';try{a.ptauLagrangeSection(0,1,new Uint8Array(128),2,2,1,0)}catch(e){m=e.message}if(!/bad argument/.test(m)){console.log('first > top accepted');process.exit(5)}"
          "m='';try{a.ptauLagrangeSection(0,1,new Uint8Array(128),2,0,29,0)}catch(e){m=e.message}if(!/bad argument/.test(m)){console.log('top 29 accepted');process.exit(6)}"
          "if(a.deviceCount()!==0){console.log('ok device');process.exit(0)}"
          "try{a.ptauLagrangeSection(0,1,new Uint8Array(128),2,0,1,0);console.log('no throw');process.exit(7)}"
          "catch(e){if(!/no HIP device/.test(e.message)){console.log(e.message);process.exit(8)}}console.log('ok')") % ADDON
    r = subprocess.run([NODE, "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


@need_node
@need_bundle
def test_the_js_driver_against_the_references_live_functions_without_a_device():
    r = subprocess.run([NODE] + FLAGS + [os.path.join(ROOT, "tests", "js", "ptau_prepare_cpu.js")], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-6000:] + r.stderr[-2000:]


@pytest.mark.gpu
@need_node
@need_bundle
def test_prepare_phase2_and_convert_through_the_addon_match_the_reference():
    r = subprocess.run([NODE] + FLAGS + [os.path.join(ROOT, "tests", "js", "ptau_prepare_gpu.js")], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-6000:] + r.stderr[-2000:]
