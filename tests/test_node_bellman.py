"""zKey.exportBellman / bellmanContribute / importBellman from Node: the addon's bellmanHSection, and js/groth16_bellman_native.js behind
registerAll(snarkjs, {bellman: true}).

 * not gpu: the addon exports the call, refuses bad arguments and fails loudly ("no HIP device") without a device; tests/js/bellman_cpu.js holds the JS driver to
   the reference's live functions under the pinned random stream on both curves and both circuits, logger lines included, with the reference's curve object in
   place of the device calls, holds it to the committed golden files and hashes, and shows that refused calls give the reference's outcome and that each
   hand-over case (a file cut short, a file that is no zkey, a section 10 cut short, an empty entropy, an unknown curve) reaches the saved function (bundle
   staged in oracle/_ref/).
 * gpu: tests/js/bellman_gpu.js runs the three functions unpatched and patched in one process and compares bytes, returned values and lines.
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
    js = ("const a=require(%r);if(typeof a.bellmanHSection!=='function'){console.log('missing');process.exit(3)}let m='';"
          "try{a.bellmanHSection(0,new Uint8Array(128),1,2)}catch(e){m=e.message}if(!/bad argument/.test(m)){console.log('direction 2 accepted');process.exit(4)}"
          "m='';try{a.bellmanHSection(5,new Uint8Array(128),1,0)}catch(e){m=e.message}if(!/bad argument/.test(m)){console.log('curve 5 accepted');process.exit(5)}"
          "m='';try{a.bellmanHSection(0,new Uint8Array(128),-1,0)}catch(e){m=e.message}if(!/bad argument/.test(m)){console.log('log_n -1 accepted');process.exit(6)}"
          "if(a.deviceCount()!==0){console.log('ok device');process.exit(0)}"
          "try{a.bellmanHSection(0,new Uint8Array(128),1,0);console.log('no throw');process.exit(7)}"
          "catch(e){if(!/no HIP device/.test(e.message)){console.log(e.message);process.exit(8)}}console.log('ok')") % ADDON
    r = subprocess.run([NODE, "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


@need_node
@need_bundle
def test_the_js_driver_against_the_references_live_functions_without_a_device():
    r = subprocess.run([NODE] + FLAGS + [os.path.join(ROOT, "tests", "js", "bellman_cpu.js")], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-6000:] + r.stderr[-2000:]
    assert "FAIL" not in r.stdout and r.stdout.count("the reference's bytes, returned value and lines") == 12
    assert r.stdout.count("the golden file and hash") == 4 and r.stdout.count("importBellman of it: the recorded key") == 4
    assert r.stdout.count("handed over before any device work") == 8 and r.stdout.count("refused before any device work") == 10
    assert r.stdout.count("BellmanRefusal with handOver") == 8 and r.stdout.count("an empty entropy reaches the saved function") == 2


@pytest.mark.gpu
@need_node
@need_bundle
def test_the_three_functions_through_the_addon_match_the_reference():
    r = subprocess.run([NODE] + FLAGS + [os.path.join(ROOT, "tests", "js", "bellman_gpu.js")], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-6000:] + r.stderr[-2000:]
    assert "FAIL" not in r.stdout and r.stdout.count("the reference's verifyFromInit accepts the key imported on the device") == 4
