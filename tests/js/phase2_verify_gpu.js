// tests/js/phase2_verify_gpu.js — snarkjs.zKey.verifyFromInit / verifyFromR1cs on the device through the real addon (tests/test_node_phase2_verify.py). Per
// curve, in ONE process, every case runs unpatched and under registerAll(snarkjs, { phase2Verify: true }):
//   1  registerAll(snarkjs) leaves the two functions the reference's; { phase2Verify: true } replaces them
//   2  verifyFromInit on the golden chain (c1, b2, c3 and the edge key), on a key with two L points swapped and on the full key against the edge init key:
//      the same verdict and the same lines to console.log and the logger, debug lines included
//   3  verifyFromR1cs on the golden c3 key and against the edge circuit: the same verdict and the same lines above debug level (the device newZKey logs
//      none of the reference's progress lines)
//   4  a PLONK key throws the reference's message; unregister restores the reference's functions
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/phase2_verify_gpu.js
"use strict";
const path = require("path");
const L = require("./phase2_verify_lib.js");
process.env.NTHREADS = process.env.NTHREADS || "8";
const snarkjs = require(path.join(L.ROOT, "oracle", "ref_shim.js"));
L.subtleShim();
const { registerAll, unregister } = require(path.join(L.ROOT, "snarkjs_amd", "js", "register.js"));
const setupN = require(path.join(L.ROOT, "snarkjs_amd", "js", "groth16_setup_native.js"));
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }
const loud = (lines) => lines.filter((x) => x[0] !== "debug");

async function runAll(name, cv) {
    const s1 = 2 * cv.n8q, ptau = L.G(`setup_${name}_p8.ptau`), init = L.G(`setup_${name}_full.zkey`), edge = L.G(`setup_${name}_edge.zkey`), c3 = L.G(`phase2_${name}_full_c3.zkey`);
    const out = {};
    for (const [label, i, k] of [["c1", init, L.G(`phase2_${name}_full_c1.zkey`)], ["b2", init, L.G(`phase2_${name}_full_b2.zkey`)], ["c3", init, c3], ["edge c1", edge, L.G(`phase2_${name}_edge_c1.zkey`)],
                                 ["swapped L", init, L.withSection(c3, 8, (b) => L.swapPoints(b, s1, (p) => p.some((x) => x)))], ["swapped init", edge, c3]])
        out["verifyFromInit " + label] = await L.capture((logger) => snarkjs.zKey.verifyFromInit(i, ptau, k, logger));
    for (const [label, r] of [["c3", L.G(`setup_${name}_full.r1cs`)], ["another circuit", L.G(`setup_${name}_edge.r1cs`)]]) {
        const res = await L.capture((logger) => snarkjs.zKey.verifyFromR1cs(r, ptau, c3, logger));
        res.lines = loud(res.lines);
        out["verifyFromR1cs " + label] = res;
    }
    out["a PLONK key"] = await L.capture((logger) => snarkjs.zKey.verifyFromInit(init, ptau, L.G("plonk_bn128_small.zkey"), logger));
    return out;
}
const WANT = { "verifyFromInit c1": true, "verifyFromInit b2": true, "verifyFromInit c3": true, "verifyFromInit edge c1": true, "verifyFromInit swapped L": false,
               "verifyFromInit swapped init": false, "verifyFromR1cs c3": true, "verifyFromR1cs another circuit": false, "a PLONK key": undefined };

async function main() {
    const orig = { verifyFromInit: snarkjs.zKey.verifyFromInit, verifyFromR1cs: snarkjs.zKey.verifyFromR1cs };
    for (const name of ["bn128", "bls12381"]) {
        const cv = setupN.CURVES.find((c) => c.name === name);
        await snarkjs.curves.getCurveFromName(name);
        const ref = await runAll(name, cv);
        await registerAll(snarkjs);
        check(`${name}: registerAll(snarkjs) keeps the reference's verifyFromInit and verifyFromR1cs`, snarkjs.zKey.verifyFromInit === orig.verifyFromInit && snarkjs.zKey.verifyFromR1cs === orig.verifyFromR1cs);
        await registerAll(snarkjs, { phase2Verify: true });
        check(`${name}: { phase2Verify: true } replaces them`, snarkjs.zKey.verifyFromInit !== orig.verifyFromInit && snarkjs.zKey.verifyFromR1cs !== orig.verifyFromR1cs);
        const dev = await runAll(name, cv);
        for (const k of Object.keys(WANT)) {
            check(`${name}: ${k}: the reference's verdict is the expected one`, ref[k].result === WANT[k], JSON.stringify([ref[k].result, ref[k].error]));
            check(`${name}: ${k}: the same verdict or thrown message`, dev[k].result === ref[k].result && dev[k].error === ref[k].error, JSON.stringify([dev[k].result, dev[k].error, ref[k].error]));
            check(`${name}: ${k}: the same lines`, L.sameLines(dev[k].lines, ref[k].lines), JSON.stringify(dev[k].lines) + " / " + JSON.stringify(ref[k].lines));
        }
        check(`${name}: a PLONK key: the reference's message`, dev["a PLONK key"].error === "zkey file is not groth16", dev["a PLONK key"].error);
        check(`${name}: swapped L: the reference's line`, JSON.stringify(loud(dev["verifyFromInit swapped L"].lines)) === JSON.stringify([["error", "L section does not match"]]));
        unregister(snarkjs);
        for (const c of ["bn128", "bls12381"]) unregister(await snarkjs.curves.getCurveFromName(c));      // registerAll patched both curve objects
        check(`${name}: unregister restores the reference's functions`, snarkjs.zKey.verifyFromInit === orig.verifyFromInit && snarkjs.zKey.verifyFromR1cs === orig.verifyFromR1cs);
    }
    console.log(fails ? `${fails} FAILED` : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.error(e); process.exit(1); });
