// tests/js/setup_gpu.js — snarkjs.zKey.newZKey on the device through the real addon (tests/test_gpu_groth16_setup.py).
//   1  registerAll(snarkjs) and { fused: true } leave snarkjs.zKey.newZKey the reference's
//   2  registerAll(snarkjs, { setup: true }): newZKey on the BN254 edge fixture writes the golden key (path and fastfile mem target) and returns its csHash
//   3  the reference's refusals come back as -1 with its logger.error
//   4  unregister(snarkjs) restores the reference's function, which still produces the same key
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/setup_gpu.js
"use strict";
const fs = require("fs"), os = require("os"), path = require("path");
const ROOT = path.join(__dirname, "..", "..");
process.env.NTHREADS = process.env.NTHREADS || "8";
const snarkjs = require(path.join(ROOT, "oracle", "ref_shim.js"));
const { registerAll, unregister, uninstallFused } = require(path.join(ROOT, "snarkjs_amd", "js", "register.js"));
const G = (f) => path.join(ROOT, "tests", "golden", f);
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }
const same = (a, b) => Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;

async function main() {
    const orig = snarkjs.zKey.newZKey;
    const golden = new Uint8Array(fs.readFileSync(G("setup_bn128_edge.zkey")));
    const wantHash = JSON.parse(fs.readFileSync(G("setup_golden.json"), "utf8"))["setup_bn128_edge.zkey"].csHash;
    await registerAll(snarkjs);
    check("registerAll(snarkjs) keeps the reference's newZKey", snarkjs.zKey.newZKey === orig);
    await registerAll(snarkjs, { fused: true });
    check("{ fused: true } keeps the reference's newZKey", snarkjs.zKey.newZKey === orig);
    await uninstallFused(snarkjs);
    await registerAll(snarkjs, { setup: true });
    check("{ setup: true } replaces newZKey", snarkjs.zKey.newZKey !== orig);
    const tmp = path.join(fs.mkdtempSync(path.join(os.tmpdir(), "zkmi-setup-")), "k.zkey");
    let h = await snarkjs.zKey.newZKey(G("setup_bn128_edge.r1cs"), G("setup_bn128_p8.ptau"), tmp);
    check("newZKey to a path: the golden key", same(new Uint8Array(fs.readFileSync(tmp)), golden));
    check("newZKey returns csHash", Buffer.from(h).toString("hex") === wantHash);
    const mem = { type: "mem" };
    h = await snarkjs.zKey.newZKey(new Uint8Array(fs.readFileSync(G("setup_bn128_edge.r1cs"))), { type: "mem", data: new Uint8Array(fs.readFileSync(G("setup_bn128_p8.ptau"))) }, mem);
    check("newZKey from bytes to a mem descriptor: the golden key", same(mem.data, golden) && Buffer.from(h).toString("hex") === wantHash);
    const errs = [];
    const rc = await snarkjs.zKey.newZKey(G("setup_bls12381_edge.r1cs"), G("setup_bn128_p8.ptau"), { type: "mem" }, { error: (m) => errs.push(m), info() {}, debug() {} });
    check("curve mismatch: -1 and the reference's message", rc === -1 && errs[0] === "r1cs curve does not match powers of tau ceremony curve", JSON.stringify(errs));
    unregister(snarkjs);
    check("unregister(snarkjs) restores the reference's newZKey", snarkjs.zKey.newZKey === orig);
    const ref = { type: "mem" };
    // the reference here is its browser bundle, which reads a string as a URL: hand it bytes
    const refHash = await snarkjs.zKey.newZKey(new Uint8Array(fs.readFileSync(G("setup_bn128_edge.r1cs"))), new Uint8Array(fs.readFileSync(G("setup_bn128_p8.ptau"))), ref);
    check("the reference path produces the golden key", same(ref.data, golden) && Buffer.from(refHash).toString("hex") === wantHash);
    fs.unlinkSync(tmp);
    console.log(fails ? `${fails} FAILED` : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.error(e); process.exit(1); });
