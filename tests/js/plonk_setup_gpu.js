// tests/js/plonk_setup_gpu.js — snarkjs.plonk.setup on the device through the real addon (tests/test_gpu_plonk_setup.py).
//   1  registerAll(snarkjs) and { setup: true } leave snarkjs.plonk.setup the reference's
//   2  registerAll(snarkjs, { plonkSetup: true }): plonk.setup on the BN254 edge fixture writes the golden key (path and fastfile mem target)
//   3  the reference's refusals come back as -1 with its logger.error
//   4  unregister(snarkjs) restores the reference's function, which still produces the same key
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/plonk_setup_gpu.js
"use strict";
const fs = require("fs"), os = require("os"), path = require("path");
const ROOT = path.join(__dirname, "..", "..");
process.env.NTHREADS = process.env.NTHREADS || "8";
const snarkjs = require(path.join(ROOT, "oracle", "ref_shim.js"));
const { registerAll, unregister } = require(path.join(ROOT, "snarkjs_amd", "js", "register.js"));
const G = (f) => path.join(ROOT, "tests", "golden", f);
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }
const same = (a, b) => Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;

async function main() {
    const orig = snarkjs.plonk.setup, origNew = snarkjs.zKey.newZKey;
    const golden = new Uint8Array(fs.readFileSync(G("plonk_setup_bn128_edge.zkey")));
    await registerAll(snarkjs);
    check("registerAll(snarkjs) keeps the reference's plonk.setup", snarkjs.plonk.setup === orig);
    await registerAll(snarkjs, { setup: true });
    check("{ setup: true } keeps the reference's plonk.setup", snarkjs.plonk.setup === orig && snarkjs.zKey.newZKey !== origNew);
    await registerAll(snarkjs, { plonkSetup: true });
    check("{ plonkSetup: true } replaces plonk.setup", snarkjs.plonk.setup !== orig);
    const tmp = path.join(fs.mkdtempSync(path.join(os.tmpdir(), "zkmi-plonk-setup-")), "k.zkey");
    const logs = [];
    const logger = { error: (m) => logs.push("ERROR " + m), info: (m) => logs.push(m), debug() {} };
    let rc = await snarkjs.plonk.setup(G("setup_bn128_edge.r1cs"), G("setup_bn128_p8.ptau"), tmp, logger);
    check("plonk.setup to a path: the golden key", rc === undefined && same(new Uint8Array(fs.readFileSync(tmp)), golden));
    check("the reference's log lines", logs.join("|") === "Reading r1cs|Plonk constraints: 178|Setup Finished", logs.join("|"));
    const mem = { type: "mem" };
    rc = await snarkjs.plonk.setup(new Uint8Array(fs.readFileSync(G("setup_bn128_edge.r1cs"))), { type: "mem", data: new Uint8Array(fs.readFileSync(G("setup_bn128_p8.ptau"))) }, mem);
    check("plonk.setup from bytes to a mem descriptor: the golden key", rc === undefined && same(mem.data, golden));
    let errs = [];
    const elog = { error: (m) => errs.push(m), info() {}, debug() {} };
    rc = await snarkjs.plonk.setup(G("setup_bls12381_edge.r1cs"), G("setup_bn128_p8.ptau"), { type: "mem" }, elog);
    check("curve mismatch: -1 and the reference's message", rc === -1 && errs[0] === "r1cs curve does not match powers of tau ceremony curve", JSON.stringify(errs));
    errs = [];
    rc = await snarkjs.plonk.setup(G("setup_bn128_full.r1cs"), G("setup_bn128_p8.ptau"), { type: "mem" }, elog);
    check("too big: -1 and the reference's message", rc === -1 && errs[0] === "circuit too big for this power of tau ceremony. 1268 > 2**8", JSON.stringify(errs));
    unregister(snarkjs);
    check("unregister(snarkjs) restores the reference's plonk.setup and newZKey", snarkjs.plonk.setup === orig && snarkjs.zKey.newZKey === origNew);
    const ref = { type: "mem" };
    // the reference here is its browser bundle, which reads a string as a URL: hand it bytes
    await snarkjs.plonk.setup(new Uint8Array(fs.readFileSync(G("setup_bn128_edge.r1cs"))), new Uint8Array(fs.readFileSync(G("setup_bn128_p8.ptau"))), ref);
    check("the reference path produces the golden key", same(ref.data, golden));
    fs.unlinkSync(tmp);
    console.log(fails ? `${fails} FAILED` : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.error(e); process.exit(1); });
