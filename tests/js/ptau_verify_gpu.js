// tests/js/ptau_verify_gpu.js — snarkjs.powersOfTau.verify on the device through the real addon (tests/test_node_ptau_verify.py). Per curve, in ONE process,
// every case runs unpatched and under registerAll(snarkjs, { ptauVerify: true }):
//   1  registerAll(snarkjs) leaves the function the reference's; { ptauVerify: true } replaces it
//   2  the p6 ceremony prepared and raw, its truncation to power 4, two tauG1 points swapped and two points of the top block of section 12 swapped (cases of
//      tests/golden/ptau_verify_golden.json): the same verdict and the same info / warn / error lines
//   3  a Groth16 zkey throws "Invalid File format"; unregister restores the reference's function
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/ptau_verify_gpu.js
"use strict";
const path = require("path");
const L = require("./ptau_verify_lib.js");
process.env.NTHREADS = process.env.NTHREADS || "8";
const snarkjs = require(path.join(L.ROOT, "oracle", "ref_shim.js"));
L.subtleShim();
const { registerAll, unregister } = require(path.join(L.ROOT, "snarkjs_amd", "js", "register.js"));
const setupN = require(path.join(L.ROOT, "snarkjs_amd", "js", "groth16_setup_native.js"));
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }
const LABELS = ["p6 prepared unpatched", "p6 raw unpatched", "truncated to power 4", "tauG1 points 3 and 5 swapped", "two points of the top block of section 12 swapped", "a Groth16 zkey"];

async function runAll(name, cv) {
    const out = {};
    for (const c of L.INDEX.cases.filter((x) => x.curve === name && LABELS.includes(x.label))) {
        const raw = L.caseFile(c, cv.n8q);
        out[c.label] = await L.capture((logger) => snarkjs.powersOfTau.verify({ type: "mem", data: raw }, logger));
        out[c.label].recorded = c;
    }
    return out;
}

async function main() {
    const orig = snarkjs.powersOfTau.verify;
    for (const name of ["bn128", "bls12381"]) {
        const cv = setupN.CURVES.find((c) => c.name === name);
        await snarkjs.curves.getCurveFromName(name);
        const ref = await runAll(name, cv);
        await registerAll(snarkjs);
        check(`${name}: registerAll(snarkjs) keeps the reference's powersOfTau.verify`, snarkjs.powersOfTau.verify === orig);
        await registerAll(snarkjs, { ptauVerify: true });
        check(`${name}: { ptauVerify: true } replaces it`, snarkjs.powersOfTau.verify !== orig);
        const dev = await runAll(name, cv);
        check(`${name}: every case ran`, Object.keys(ref).length === LABELS.length && Object.keys(dev).length === LABELS.length);
        for (const k of Object.keys(ref)) {
            const c = ref[k].recorded;
            check(`${name}: ${k}: the reference's answer is the recorded one`, ref[k].result === c.verdict && ref[k].error === c.throws && L.sameLines(ref[k].lines, c.lines));
            check(`${name}: ${k}: the same verdict or thrown message`, dev[k].result === ref[k].result && L.afterName(dev[k].error) === L.afterName(ref[k].error), JSON.stringify([dev[k].result, dev[k].error, ref[k].error]));
            check(`${name}: ${k}: the same lines`, L.sameLines(dev[k].lines, ref[k].lines), JSON.stringify(dev[k].lines) + " / " + JSON.stringify(ref[k].lines));
        }
        unregister(snarkjs);
        for (const c of ["bn128", "bls12381"]) unregister(await snarkjs.curves.getCurveFromName(c));      // registerAll patched both curve objects
        check(`${name}: unregister restores the reference's function`, snarkjs.powersOfTau.verify === orig);
    }
    console.log(fails ? `${fails} FAILED` : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.error(e); process.exit(1); });
