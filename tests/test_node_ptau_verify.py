"""powersOfTau.verify from Node: the addon's ptauSectionCheck and blake2bResume and js/powersoftau_verify_native.js behind registerAll(snarkjs, {ptauVerify: true}).

 * not gpu: the addon exports the two calls; blake2bResume answers without a device and gives Python's answer; ptauSectionCheck refuses bad arguments and fails
   loudly ("no HIP device") without a device; tests/js/ptau_verify_cpu.js holds the JS driver's parsing, order and lines to the reference's own
   powersOfTau.verify on every case of tests/golden/ptau_verify_golden.json, with the reference's curve object in place of the device calls (bundle staged in
   oracle/_ref/).
 * gpu: tests/js/ptau_verify_gpu.js runs the function unpatched and patched in one process and compares verdicts and lines.
"""
import hashlib
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
    msg = bytes(range(200)) * 3
    want = hashlib.blake2b(msg).hexdigest()
    # a hasher that has taken nothing: the initial state words, an empty buffer, length and position zero
    js = ("const a=require(%r);for(const f of ['ptauSectionCheck','blake2bResume'])if(typeof a[f]!=='function'){console.log('missing '+f);process.exit(3)}"
          "const iv=[0x6a09e667f3bcc908n^0x01010040n,0xbb67ae8584caa73bn,0x3c6ef372fe94f82bn,0xa54ff53a5f1d36f1n,0x510e527fade682d1n,0x9b05688c2b3e6c1fn,0x1f83d9abfb41bd6bn,0x5be0cd19137e2179n];"
          "const p=new Uint8Array(216),dv=new DataView(p.buffer);iv.forEach((v,i)=>dv.setBigUint64(128+8*i,v,true));"
          "const msg=new Uint8Array(600);for(let i=0;i<600;i++)msg[i]=i%%200;"
          "if(Buffer.from(a.blake2bResume(p,msg)).toString('hex')!==%r){console.log('blake2bResume differs');process.exit(4)}"
          "if(Buffer.from(a.blake2bResume(p,new Uint8Array(0))).toString('hex')!==%r){console.log('blake2bResume of nothing differs');process.exit(5)}"
          "let m='';try{a.blake2bResume(new Uint8Array(215),msg)}catch(e){m=e.message}if(!/bad argument/.test(m)){console.log('short state accepted');process.exit(6)}"
          "m='';try{a.ptauSectionCheck(0,3,new Uint8Array(64),1,null,0,0,new Uint8Array(32),new Uint8Array(32))}catch(e){m=e.message}"
          "if(!/bad argument/.test(m)){console.log('group 3 accepted');process.exit(7)}"
          "m='';try{a.ptauSectionCheck(0,1,new Uint8Array(64),1,null,0,0,new Uint8Array(31),new Uint8Array(32))}catch(e){m=e.message}"
          "if(!/bad argument/.test(m)){console.log('short seed accepted');process.exit(8)}"
          "if(a.deviceCount()!==0){console.log('ok device');process.exit(0)}"
          "try{a.ptauSectionCheck(0,1,new Uint8Array(128),2,null,1,0,new Uint8Array(32),new Uint8Array(32));console.log('no throw');process.exit(9)}"
          "catch(e){if(!/no HIP device/.test(e.message)){console.log(e.message);process.exit(10)}}console.log('ok')") % (
        ADDON, want, hashlib.blake2b(b"").hexdigest())
    r = subprocess.run([NODE, "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


@need_node
@need_bundle
def test_the_js_driver_against_the_references_verify_without_a_device():
    r = subprocess.run([NODE] + FLAGS + [os.path.join(ROOT, "tests", "js", "ptau_verify_cpu.js")], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-6000:] + r.stderr[-2000:]


@pytest.mark.gpu
@need_node
@need_bundle
def test_powers_of_tau_verify_through_the_addon_matches_the_reference():
    r = subprocess.run([NODE] + FLAGS + [os.path.join(ROOT, "tests", "js", "ptau_verify_gpu.js")], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-6000:] + r.stderr[-2000:]
