// tests/js/phase2_verify_cpu.js — js/groth16_phase2_verify_native.js without a device (tests/test_node_phase2_verify.py): its parsing, its order of checks
// and its lines against the reference's own zKey.verifyFromInit, with the reference's curve object in place of the three device calls (phase2_verify_lib.js:
// refDevice). Per case both run on the same three inputs; verdict (or thrown message) and every line to console.log and the logger must be equal.
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/phase2_verify_cpu.js
"use strict";
const path = require("path");
const L = require("./phase2_verify_lib.js");
process.env.NTHREADS = process.env.NTHREADS || "8";
const snarkjs = require(path.join(L.ROOT, "oracle", "ref_shim.js"));
L.subtleShim();
const verifyN = require(path.join(L.ROOT, "snarkjs_amd", "js", "groth16_phase2_verify_native.js"));
const setupN = require(path.join(L.ROOT, "snarkjs_amd", "js", "groth16_setup_native.js"));
const addon = require(path.join(L.ROOT, "snarkjs_amd", "napi", "zkmi_napi.node"));
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }

function cases(name, cv) {
    const s1 = 2 * cv.n8q, init = L.G(`setup_${name}_full.zkey`), edge = L.G(`setup_${name}_edge.zkey`), key = L.G(`phase2_${name}_full_c3.zkey`);
    const out = [["the golden key after three contributions", init, key, true], ["two L points swapped", init, L.withSection(key, 8, (b) => L.swapPoints(b, s1, (p) => p.some((x) => x))), false]];
    if (name !== "bn128") return out;
    const sec2 = L.sectionOf(key, 2), at = 4 + cv.n8q + 4 + 32 + 12, gamma2 = sec2.subarray(at + 2 * s1 + 2 * s1, at + 2 * s1 + 4 * s1);
    return out.concat([
        ["the edge key after one contribution", edge, L.G(`phase2_${name}_edge_c1.zkey`), true],
        ["a byte of the second transcript", init, L.withContribution(cv, key, 1, (c) => { c.transcript = Uint8Array.from(c.transcript); c.transcript[0] ^= 1; }), false],
        ["the beacon's iterations 10 -> 11", init, L.withContribution(cv, key, 1, (c) => { c.numIterationsExp = 11; }), false],
        ["delta2 <- gamma2", init, L.withSection(key, 2, (b) => { const o = Uint8Array.from(b); o.set(gamma2, b.length - 2 * s1); return o; }), false],
        ["the full key against the edge init key", edge, key, false],
        ["two H points swapped", init, L.withSection(key, 9, (b) => L.swapPoints(b, s1, () => true)), false],
        ["a PLONK key", init, L.G("plonk_bn128_small.zkey"), undefined],
        ["a PLONK key as the init key", L.G("plonk_bn128_small.zkey"), L.G(`phase2_${name}_full_c1.zkey`), undefined],
    ]);
}

async function main() {
    const random64 = Uint8Array.from({ length: 64 }, (_, i) => i);
    for (const name of ["bn128", "bls12381"]) {
        const curve = await snarkjs.curves.getCurveFromName(name), cv = setupN.CURVES.find((c) => c.name === name);
        const dev = L.refDevice(curve, cv, addon, verifyN.deviceOf(addon)), ptau = L.G(`setup_${name}_p8.ptau`);
        for (const [label, init, key, want] of cases(name, cv)) {
            const ref = await L.capture((logger) => snarkjs.zKey.verifyFromInit(init, ptau, key, logger));
            const got = await L.capture((logger) => verifyN.verifyFromInit(init, ptau, key, { addon, dev, random64, log: (level, text) => (level === "log" ? console.log(text) : logger[level](text)) }));
            check(`${name}: ${label}: the reference's verdict is the expected one`, ref.result === want, JSON.stringify([ref.result, ref.error]));
            check(`${name}: ${label}: the same verdict or thrown message`, got.result === ref.result && got.error === ref.error, JSON.stringify([got.result, got.error, ref.error]));
            check(`${name}: ${label}: the same lines`, L.sameLines(got.lines, ref.lines), JSON.stringify(got.lines) + " / " + JSON.stringify(ref.lines));
        }
    }
    console.log(fails ? `${fails} FAILED` : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.error(e); process.exit(1); });
