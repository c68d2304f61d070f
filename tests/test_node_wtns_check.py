"""wtns.check from Node: the addon's r1csLoad and r1csCheck, and js/wtns_check_native.js behind registerAll(snarkjs, {wtnsCheck: true}).

 * not gpu: the addon exports the two calls, refuses bad arguments and fails loudly ("no HIP device") without a device; tests/js/wtns_check_cpu.js holds the JS
   driver to the reference's LIVE function under a recording logger on every golden case, with the device calls written in plain JS, and shows that each
   hand-off case reaches the saved function before any device call (bundle staged in oracle/_ref/).
 * gpu: tests/js/wtns_check_gpu.js runs the golden cases unpatched and patched in one process through the real addon, then unregisters.
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
    js = ("const a=require(%r);for(const k of ['r1csLoad','r1csCheck'])if(typeof a[k]!=='function'){console.log('missing '+k);process.exit(3)}"
          "const sec=new Uint8Array(12);let m='';"
          "try{a.r1csLoad(0,sec,1,1,0)}catch(e){m=e.message}if(!/bad argument/.test(m)){console.log('key 0 accepted');process.exit(4)}"
          "m='';try{a.r1csLoad(0,'x',1,1,5)}catch(e){m=e.message}if(!/bad argument/.test(m)){console.log('a string accepted');process.exit(5)}"
          "m='';try{a.r1csCheck(5,[new Uint8Array(32),new Uint8Array(32)],1)}catch(e){m=e.message}if(!/bad argument/.test(m)){console.log('pages accepted');process.exit(6)}"
          "m='';try{a.r1csCheck(5,new Uint8Array(32),-1)}catch(e){m=e.message}if(!/bad argument/.test(m)){console.log('n = -1 accepted');process.exit(7)}"
          "m='';try{a.call('zkmi_r1cs_release')}catch(e){m=e.message}if(!/too few arguments/.test(m)){console.log('release without a key');process.exit(8)}"
          "if(a.deviceCount()!==0){console.log('ok device');process.exit(0)}"
          "try{a.r1csLoad(0,sec,1,1,5);console.log('no throw');process.exit(9)}"
          "catch(e){if(!/no HIP device/.test(e.message)){console.log(e.message);process.exit(10)}}"
          "try{a.r1csCheck(5,new Uint8Array(32),1);console.log('no throw');process.exit(11)}"
          "catch(e){if(!/no HIP device/.test(e.message)){console.log(e.message);process.exit(12)}}console.log('ok')") % ADDON
    r = subprocess.run([NODE, "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


@need_node
@need_bundle
def test_the_js_driver_against_the_references_live_function_without_a_device():
    r = subprocess.run([NODE] + FLAGS + [os.path.join(ROOT, "tests", "js", "wtns_check_cpu.js")], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-6000:] + r.stderr[-2000:]
    assert "FAIL" not in r.stdout
    # per curve 6 cases the reference refuses or reads beyond a buffer for, with and without a logger, and 15 that run on the device calls
    assert r.stdout.count("handed over before any device work") == 24
    assert r.stdout.count("one load, one check, one release, nothing handed over") == 60
    assert r.stdout.count("the reference's thrown message and lines") == 16


@pytest.mark.gpu
@need_node
@need_bundle
def test_wtns_check_through_the_addon_matches_the_reference():
    r = subprocess.run([NODE] + FLAGS + [os.path.join(ROOT, "tests", "js", "wtns_check_gpu.js")], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-6000:] + r.stderr[-2000:]
    assert "FAIL" not in r.stdout and r.stdout.count("the reference's lines") == 72 and r.stdout.count("a batch of five") == 2
