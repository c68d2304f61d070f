// tests/js/phase2_gpu.js — snarkjs.zKey.contribute / zKey.beacon on the device through the real addon (tests/test_node_phase2.py). Per curve, in ONE process:
//   1  registerAll(snarkjs) leaves zKey.contribute / beacon the reference's
//   2  the chain contribute('c1') -> beacon('b2', 0102..1f, 10) -> contribute(undefined) from setup_<curve>_full.zkey, unpatched, with reseed() before it
//   3  the same chain under registerAll(snarkjs, { phase2: true }), reseed() before it: the same key bytes and the same returned hashes at every step
//   4  beacon's refusals: false and the reference's logger.error; a PLONK key throws the reference's message
//   5  unregister: the reference's own verifyFromInit and verifyFromR1cs accept the device-made key, and refuse it against another initial key
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/phase2_gpu.js
"use strict";
const fs = require("fs"), path = require("path"), nodeCrypto = require("crypto");
const ROOT = path.join(__dirname, "..", "..");
process.env.NTHREADS = process.env.NTHREADS || "8";
const snarkjs = require(path.join(ROOT, "oracle", "ref_shim.js"));
const { registerAll, unregister } = require(path.join(ROOT, "snarkjs_amd", "js", "register.js"));
const G = (f) => new Uint8Array(fs.readFileSync(path.join(ROOT, "tests", "golden", f)));
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }
const same = (a, b) => Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;
const hex = (b) => Buffer.from(b).toString("hex");
const BEACON = Array.from({ length: 31 }, (_, i) => (i + 1).toString(16).padStart(2, "0")).join("");
const quiet = { error() {}, info() {}, debug() {}, warn() {} };
// the reference's browser build hashes the beacon through crypto.subtle.digest, which the shim's crypto object lacks
globalThis.crypto.subtle = { digest: async (alg, ab) => { const d = nodeCrypto.createHash("sha256").update(Buffer.from(ab)).digest(); return d.buffer.slice(d.byteOffset, d.byteOffset + d.byteLength); } };

async function chain(curveName) {
    snarkjs.reseed();
    const keys = [], hashes = [];
    let cur = { type: "mem", data: G(`setup_${curveName}_full.zkey`) };
    const steps = [(o, n) => snarkjs.zKey.contribute(o, n, "c1", "Entropy1"), (o, n) => snarkjs.zKey.beacon(o, n, "b2", BEACON, 10), (o, n) => snarkjs.zKey.contribute(o, n, undefined, "Entropy3")];
    for (const f of steps) {
        const next = { type: "mem" };
        hashes.push(hex(await f(cur, next)));
        keys.push(next.data instanceof Uint8Array ? next.data : next.data.slice(0, next.data.byteLength));
        cur = { type: "mem", data: keys[keys.length - 1] };
    }
    return { keys, hashes };
}

async function main() {
    const orig = { contribute: snarkjs.zKey.contribute, beacon: snarkjs.zKey.beacon };
    for (const name of ["bn128", "bls12381"]) {
        await snarkjs.curves.getCurveFromName(name);
        const ref = await chain(name);
        await registerAll(snarkjs);
        check(`${name}: registerAll(snarkjs) keeps the reference's contribute and beacon`, snarkjs.zKey.contribute === orig.contribute && snarkjs.zKey.beacon === orig.beacon);
        await registerAll(snarkjs, { phase2: true });
        check(`${name}: { phase2: true } replaces them`, snarkjs.zKey.contribute !== orig.contribute && snarkjs.zKey.beacon !== orig.beacon);
        const dev = await chain(name);
        for (let i = 0; i < 3; i++) check(`${name}: step ${i + 1}: the same key and the same contribution hash`, same(dev.keys[i], ref.keys[i]) && dev.hashes[i] === ref.hashes[i], dev.hashes[i] + " " + ref.hashes[i]);
        if (name === "bn128") {
            const errs = [], log = Object.assign({}, quiet, { error: (m) => errs.push(m) });
            const key = { type: "mem", data: dev.keys[0] };
            const r1 = await snarkjs.zKey.beacon(key, { type: "mem" }, "x", "012", 10, log), r2 = await snarkjs.zKey.beacon(key, { type: "mem" }, "x", "0102", 9, log);
            check("beacon refusals: false and the reference's messages", r1 === false && r2 === false && errs[0] === "Invalid Beacon Hash. (It must be a valid hexadecimal sequence)" &&
                  errs[1] === "Invalid numIterationsExp. (Must be between 10 and 63)", JSON.stringify(errs));
            let msg = "";
            try { await snarkjs.zKey.contribute({ type: "mem", data: G("plonk_bn128_small.zkey") }, { type: "mem" }, "x", "e"); } catch (e) { msg = e.message; }
            check("a PLONK key: the reference's message", msg === "zkey file is not groth16", msg);
        }
        unregister(snarkjs);
        for (const c of ["bn128", "bls12381"]) unregister(await snarkjs.curves.getCurveFromName(c));      // registerAll patched both curve objects
        check(`${name}: unregister restores the reference's functions`, snarkjs.zKey.contribute === orig.contribute && snarkjs.zKey.beacon === orig.beacon);
        const init = G(`setup_${name}_full.zkey`), ptau = G(`setup_${name}_p8.ptau`), r1cs = G(`setup_${name}_full.r1cs`), made = dev.keys[2];
        check(`${name}: the reference's verifyFromInit accepts the device-made key`, (await snarkjs.zKey.verifyFromInit(init, ptau, made, quiet)) === true);
        check(`${name}: the reference's verifyFromR1cs accepts it`, (await snarkjs.zKey.verifyFromR1cs(r1cs, ptau, made, quiet)) === true);
        check(`${name}: verifyFromInit refuses it against another initial key`, (await snarkjs.zKey.verifyFromInit(G(`setup_${name}_edge.zkey`), ptau, made, quiet)) === false);
    }
    console.log(fails ? `${fails} FAILED` : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.error(e); process.exit(1); });
