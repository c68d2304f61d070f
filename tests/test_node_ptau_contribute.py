"""powersOfTau.newAccumulator / contribute / beacon from Node: the addon's ptauContributeSection and blake2b512Partial, and js/powersoftau_contribute_native.js
behind registerAll(snarkjs, {ptauContribute: true}).

 * not gpu: the addon exports the calls, refuses bad arguments and fails loudly ("no HIP device") without a device; tests/js/ptau_contribute_cpu.js holds the JS
   driver to the reference's live functions under the pinned random stream on the power-1 and power-5 chains of both curves, with the reference's curve object
   in place of the device call, has the reference's own powersOfTau.verify accept the ceremony the driver made, and shows that refused calls give the
   reference's outcome and files that are not well-formed reach the saved function (bundle staged in oracle/_ref/).
 * gpu: tests/js/ptau_contribute_gpu.js runs the three functions unpatched and patched in one process and compares bytes.
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
    js = ("const a=require(%r);for(const k of ['ptauContributeSection','blake2b512Partial'])if(typeof a[k]!=='function'){console.log('missing '+k);process.exit(3)}"
          "const one=new Uint8Array(32);let m='';"
          "try{a.ptauContributeSection(0,3,new Uint8Array(128),2,one,one)}catch(e){m=e.message}if(!/bad argument/.test(m)){console.log('group 3 accepted');process.exit(4)}"
          "m='';try{a.ptauContributeSection(0,1,new Uint8Array(128),2,new Uint8Array(31),one)}catch(e){m=e.message}if(!/bad argument/.test(m)){console.log('short scalar accepted');process.exit(5)}"
          "m='';try{a.blake2b512Partial(new Uint8Array(4))}catch(e){m=e.message}if(!/bad argument/.test(m)){console.log('a bare buffer accepted');process.exit(6)}"
          "const p=a.blake2b512Partial([new Uint8Array(3),new Uint8Array(0)]);if(p.length!==216||p[128+72]!==3){console.log('partial state');process.exit(9)}"
          "if(a.deviceCount()!==0){console.log('ok device');process.exit(0)}"
          "try{a.ptauContributeSection(0,1,new Uint8Array(128),2,one,one);console.log('no throw');process.exit(7)}"
          "catch(e){if(!/no HIP device/.test(e.message)){console.log(e.message);process.exit(8)}}console.log('ok')") % ADDON
    r = subprocess.run([NODE, "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


@need_node
@need_bundle
def test_the_js_driver_against_the_references_live_functions_without_a_device():
    r = subprocess.run([NODE] + FLAGS + [os.path.join(ROOT, "tests", "js", "ptau_contribute_cpu.js")], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-6000:] + r.stderr[-2000:]
    assert r.stdout.count("the reference's verify accepts the ceremony made here") == 4 and "FAIL" not in r.stdout


@pytest.mark.gpu
@need_node
@need_bundle
def test_the_three_functions_through_the_addon_match_the_reference():
    r = subprocess.run([NODE] + FLAGS + [os.path.join(ROOT, "tests", "js", "ptau_contribute_gpu.js")], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-6000:] + r.stderr[-2000:]
