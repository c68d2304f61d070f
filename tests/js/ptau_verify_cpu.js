// tests/js/ptau_verify_cpu.js — js/powersoftau_verify_native.js without a device (tests/test_node_ptau_verify.py): its parsing, its order of checks and its
// lines against the reference's own powersOfTau.verify on every case of tests/golden/ptau_verify_golden.json, with the reference's curve object in place of
// the device calls (ptau_verify_lib.js: refDevice). Per case both run on the same bytes; the reference's live answer must be the recorded one, and the driver's
// verdict (or thrown message, after the file's name) and its info / warn / error lines must be the reference's.
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/ptau_verify_cpu.js
"use strict";
const path = require("path");
const L = require("./ptau_verify_lib.js");
process.env.NTHREADS = process.env.NTHREADS || "8";
const snarkjs = require(path.join(L.ROOT, "oracle", "ref_shim.js"));
L.subtleShim();
const verifyN = require(path.join(L.ROOT, "snarkjs_amd", "js", "powersoftau_verify_native.js"));
const setupN = require(path.join(L.ROOT, "snarkjs_amd", "js", "groth16_setup_native.js"));
const addon = require(path.join(L.ROOT, "snarkjs_amd", "napi", "zkmi_napi.node"));
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }

async function main() {
    const random32 = Uint8Array.from({ length: 32 }, (_, i) => 200 + i);
    for (const name of ["bn128", "bls12381"]) {
        const curve = await snarkjs.curves.getCurveFromName(name), cv = setupN.CURVES.find((c) => c.name === name);
        const dev = L.refDevice(curve, cv, addon, verifyN.deviceOf(addon));
        // what the reference throws at a section, after the lines before it: built here, the reference's live answer is the yardstick
        const p6raw = L.G(`ptau_${name}_p6_c3b_raw.ptau`), secs = L.split(p6raw);
        const thrown = [["no section 3", secs.filter(([t]) => t != 3)], ["section 2 twice", secs.concat(secs.filter(([t]) => t == 2))],
                        ["section 4 one byte short", secs.map(([t, b]) => [t, t == 4 ? b.subarray(0, b.length - 1) : b])], ["no section 6", secs.filter(([t]) => t != 6)]];
        for (const [what, edited] of thrown) {
            const raw = L.join(p6raw, edited), label = `${name}: ${what}`;
            const ref = await L.capture((logger) => snarkjs.powersOfTau.verify({ type: "mem", data: raw }, logger));
            const got = await L.capture((logger) => verifyN.verify(raw, { addon, dev, random32, log: (level, text) => logger[level](text) }));
            check(`${label}: the reference throws`, ref.error !== undefined && ref.result === undefined, JSON.stringify([ref.result, ref.error]));
            check(`${label}: the same thrown message`, got.result === undefined && L.afterName(got.error) === L.afterName(ref.error), JSON.stringify([got.result, got.error, ref.error]));
            check(`${label}: the same lines`, L.sameLines(got.lines, ref.lines), JSON.stringify(got.lines) + " / " + JSON.stringify(ref.lines));
        }
        for (const c of L.INDEX.cases.filter((x) => x.curve === name)) {
            const raw = L.caseFile(c, cv.n8q), label = `${name}: ${c.label}`;
            const ref = await L.capture((logger) => snarkjs.powersOfTau.verify({ type: "mem", data: raw }, logger));
            const got = await L.capture((logger) => verifyN.verify(raw, { addon, dev, random32, log: (level, text) => logger[level](text) }));
            check(`${label}: the reference's answer is the recorded one`, ref.result === c.verdict && ref.error === c.throws && L.sameLines(ref.lines, c.lines), JSON.stringify([ref.result, ref.error]));
            check(`${label}: the same verdict or thrown message`, got.result === ref.result && L.afterName(got.error) === L.afterName(ref.error), JSON.stringify([got.result, got.error, ref.error]));
            check(`${label}: the same lines`, L.sameLines(got.lines, ref.lines), JSON.stringify(got.lines) + " / " + JSON.stringify(ref.lines));
        }
    }
    console.log(fails ? `${fails} FAILED` : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.error(e); process.exit(1); });
