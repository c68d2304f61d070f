// tests/js/verify_gpu.js — batch Groth16 verification from Node on the GPU box, against the reference's own groth16.verify (the bundle staged
// into oracle/_ref/). argv[2]: a JSON file of cases written by tests/test_node_verify.py: [{vk, cases: [{label, publicSignals, proof}]}].
//   1  VerifyingKey.verifyMany verdicts == the reference's verify on every case (valid, tampered, Jacobian-form, off-subgroup)
//   2  registerAll(snarkjs, {fused: true, verify: true}): 256 concurrent snarkjs.groth16.verify calls give the reference's results and logger
//      messages, in fewer than 256 device batches; uninstallFused restores the reference's function
//   3  registerAll(snarkjs, {fused: true}) leaves snarkjs.groth16.verify as the reference's
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/verify_gpu.js cases.json
"use strict";
const fs = require("fs"), path = require("path");
const ROOT = path.join(__dirname, "..", "..");
process.env.NTHREADS = process.env.NTHREADS || "8";
const snarkjs = require(path.join(ROOT, "oracle", "ref_shim.js"));
const { registerAll, uninstallFused, unregister } = require(path.join(ROOT, "snarkjs_amd", "js", "register.js"));
const { VerifyingKey } = require(path.join(ROOT, "snarkjs_amd", "js", "groth16_verify_native.js"));
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }
function recorder() { const msgs = []; return { msgs, info: (m) => msgs.push("info:" + m), error: (m) => msgs.push("error:" + m), warn: () => {}, debug: () => {} }; }

async function main() {
    const sets = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
    const origVerify = snarkjs.groth16.verify;
    const want = [];
    for (const s of sets) {
        const w = [];
        for (const c of s.cases) { const lg = recorder(); w.push({ ok: await origVerify(s.vk, c.publicSignals, c.proof, lg), msgs: lg.msgs }); }
        want.push(w);
        const key = new VerifyingKey(s.vk, { device: 0 });
        const got = await key.verifyMany(s.cases.map((c) => c.publicSignals), s.cases.map((c) => c.proof));
        s.cases.forEach((c, i) => check(s.vk.curve + " verifyMany " + c.label, got[i] === w[i].ok, "got " + got[i] + " want " + w[i].ok));
        key.release();
    }
    // 3: fused without verify leaves verify alone
    await registerAll(snarkjs, { fused: true });
    check("fused without verify keeps the reference's verify", snarkjs.groth16.verify === origVerify);
    await uninstallFused(snarkjs);
    // 2: the drop-in
    const out = await registerAll(snarkjs, { fused: true, verify: true });
    check("verify: true replaces groth16.verify", snarkjs.groth16.verify !== origVerify);
    for (let si = 0; si < sets.length; si++) {
        const s = sets[si], calls = [], loggers = [], idx = [];
        for (let i = 0; i < 256; i++) {
            const k = i % s.cases.length, lg = recorder();
            idx.push(k); loggers.push(lg);
            calls.push(snarkjs.groth16.verify(s.vk, s.cases[k].publicSignals, s.cases[k].proof, lg));
        }
        const before = out.fused.verifier.stats.batches;
        const res = await Promise.all(calls);
        const batches = out.fused.verifier.stats.batches - before;
        check(s.vk.curve + " 256 concurrent calls: reference results", res.every((r, i) => r === want[si][idx[i]].ok));
        check(s.vk.curve + " 256 concurrent calls: reference logger messages", loggers.every((lg, i) => JSON.stringify(lg.msgs) === JSON.stringify(want[si][idx[i]].msgs)),
              JSON.stringify(loggers[0].msgs) + " vs " + JSON.stringify(want[si][idx[0]].msgs));
        check(s.vk.curve + " coalesced into " + batches + " device batches (< 256)", batches >= 1 && batches < 256);
    }
    await uninstallFused(snarkjs);
    check("uninstallFused restores the reference's verify", snarkjs.groth16.verify === origVerify);
    for (const name of ["bn128", "bls12381"]) unregister(await snarkjs.curves.getCurveFromName(name));
    console.log(fails ? "FAILED " + fails : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.log("FAIL exception", e && e.stack || e); process.exit(2); });
