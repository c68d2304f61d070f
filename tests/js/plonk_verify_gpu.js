// tests/js/plonk_verify_gpu.js — batch PLONK verification from Node on the GPU box, against the reference's own plonk.verify (the bundle staged
// into oracle/_ref/). argv[2]: a JSON file of cases written by tests/test_node_plonk_verify.py: [{vk, cases: [{label, publicSignals, proof}]}].
//   1  VerifyingKey.verifyMany verdicts == the reference's verify on every case (valid, tampered, Jacobian-form, wrong signal count)
//   2  registerAll(snarkjs, {fused: true, verify: {groth16: true, plonk: true}}): 128 concurrent snarkjs.plonk.verify calls give the reference's
//      results and logger messages, in fewer than 128 device batches; uninstallFused restores the reference's function
//   3  registerAll(snarkjs, {fused: true, verify: true}) leaves snarkjs.plonk.verify as the reference's; verifyPlonk: true replaces it alone
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/plonk_verify_gpu.js cases.json
"use strict";
const fs = require("fs"), path = require("path");
const ROOT = path.join(__dirname, "..", "..");
process.env.NTHREADS = process.env.NTHREADS || "8";
const snarkjs = require(path.join(ROOT, "oracle", "ref_shim.js"));
const { registerAll, uninstallFused, unregister } = require(path.join(ROOT, "snarkjs_amd", "js", "register.js"));
const { VerifyingKey } = require(path.join(ROOT, "snarkjs_amd", "js", "plonk_verify_native.js"));
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }
function recorder() {
    const msgs = [];
    return { msgs, info: (m) => msgs.push("info:" + m), error: (m) => msgs.push("error:" + m), warn: (m) => msgs.push("warn:" + m), debug: () => {} };
}

async function main() {
    const sets = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
    const origVerify = snarkjs.plonk.verify, origG16 = snarkjs.groth16.verify;
    const want = [];
    for (const s of sets) {
        const w = [];
        for (const c of s.cases) { const lg = recorder(); w.push({ ok: await origVerify(s.vk, c.publicSignals, c.proof, lg), msgs: lg.msgs }); }
        want.push(w);
        const key = new VerifyingKey(s.vk, { device: 0 });
        // the addon sizes a batch by the handle's own curve: a record buffer of the other curve's size is refused before anything is copied
        const otherRec = 27 * (s.vk.curve === "bn128" ? 48 : 32) + 192;
        let refused = false;
        try { await require(path.join(ROOT, "snarkjs_amd", "napi", "zkmi_napi.node")).plonkVerifyAsync(key.handle, new Uint8Array(otherRec), new Uint8Array(32 * key.nPublic), key.nPublic, 1); }
        catch (e) { refused = true; }
        check(s.vk.curve + " addon refuses a record buffer of the other curve's size", refused);
        const byCount = new Map();
        s.cases.forEach((c, i) => { const k = c.publicSignals.length; if (!byCount.has(k)) byCount.set(k, []); byCount.get(k).push(i); });
        for (const idx of byCount.values()) {
            const got = await key.verifyMany(idx.map((i) => s.cases[i].publicSignals), idx.map((i) => s.cases[i].proof));
            idx.forEach((i, j) => check(s.vk.curve + " verifyMany " + s.cases[i].label, got[j] === w[i].ok, "got " + got[j] + " want " + w[i].ok));
        }
        key.release();
    }
    // 3: verify: true alone is Groth16 only
    await registerAll(snarkjs, { fused: true, verify: true });
    check("verify: true keeps the reference's plonk.verify", snarkjs.plonk.verify === origVerify && snarkjs.groth16.verify !== origG16);
    await uninstallFused(snarkjs);
    await registerAll(snarkjs, { fused: true, verifyPlonk: true });
    check("verifyPlonk: true replaces plonk.verify alone", snarkjs.plonk.verify !== origVerify && snarkjs.groth16.verify === origG16);
    await uninstallFused(snarkjs);
    // 2: the drop-in
    const out = await registerAll(snarkjs, { fused: true, verify: { groth16: true, plonk: true } });
    check("verify: {groth16, plonk} replaces both", snarkjs.plonk.verify !== origVerify && snarkjs.groth16.verify !== origG16);
    for (let si = 0; si < sets.length; si++) {
        const s = sets[si], calls = [], loggers = [], idx = [];
        for (let i = 0; i < 128; i++) {
            const k = i % s.cases.length, lg = recorder();
            idx.push(k); loggers.push(lg);
            calls.push(snarkjs.plonk.verify(s.vk, s.cases[k].publicSignals, s.cases[k].proof, lg));
        }
        const before = out.fused.plonkVerifier.stats.batches;
        const res = await Promise.all(calls);
        const batches = out.fused.plonkVerifier.stats.batches - before;
        check(s.vk.curve + " 128 concurrent calls: reference results", res.every((r, i) => r === want[si][idx[i]].ok));
        const badLog = loggers.findIndex((lg, i) => JSON.stringify(lg.msgs) !== JSON.stringify(want[si][idx[i]].msgs));
        check(s.vk.curve + " 128 concurrent calls: reference logger messages", badLog < 0,
              badLog < 0 ? "" : s.cases[idx[badLog]].label + " " + JSON.stringify(loggers[badLog].msgs) + " vs " + JSON.stringify(want[si][idx[badLog]].msgs));
        check(s.vk.curve + " coalesced into " + batches + " device batches (< 128)", batches >= 1 && batches < 128);
        check(s.vk.curve + " without a logger", (await snarkjs.plonk.verify(s.vk, s.cases[0].publicSignals, s.cases[0].proof)) === want[si][0].ok);
    }
    await uninstallFused(snarkjs);
    check("uninstallFused restores the reference's verify", snarkjs.plonk.verify === origVerify && snarkjs.groth16.verify === origG16);
    for (const name of ["bn128", "bls12381"]) unregister(await snarkjs.curves.getCurveFromName(name));
    console.log(fails ? "FAILED " + fails : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.log("FAIL exception", e && e.stack || e); process.exit(2); });
