// tests/js/fflonk_verify_gpu.js — batch FFLONK verification from Node on the GPU box, against the reference's own fflonk.verify (the bundle staged
// into oracle/_ref/) in the same process. argv[2]: a JSON file of cases written by tests/test_node_fflonk_verify.py:
// [{vk, cases: [{label, publicSignals, proof}]}] (a set may carry a key whose C0 is off the curve).
//   1  VerifyingKey.verifyMany verdicts == the reference's verify on every case (valid, tampered, Jacobian-form, a + r, inv changed, wrong signal count)
//   2  registerAll(snarkjs, {fused: true, verify: {fflonk: true}}): 128 concurrent snarkjs.fflonk.verify calls give the reference's results and its
//      final logger message (level and text; after a pairing verdict the line before "FFLONK VERIFIER FINISHED"), STARTED first, in fewer than 128
//      device batches; uninstallFused restores the reference's function
//   3  registerAll(snarkjs, {fused: true, verify: true}) leaves snarkjs.fflonk.verify as the reference's; verifyFflonk: true replaces it alone
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/fflonk_verify_gpu.js cases.json
"use strict";
const fs = require("fs"), path = require("path");
const ROOT = path.join(__dirname, "..", "..");
process.env.NTHREADS = process.env.NTHREADS || "8";
const snarkjs = require(path.join(ROOT, "oracle", "ref_shim.js"));
const { registerAll, uninstallFused, unregister } = require(path.join(ROOT, "snarkjs_amd", "js", "register.js"));
const { VerifyingKey } = require(path.join(ROOT, "snarkjs_amd", "js", "fflonk_verify_native.js"));
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }
function recorder() {
    const msgs = [];
    return { msgs, info: (m) => msgs.push("info:" + m), error: (m) => msgs.push("error:" + m), warn: (m) => msgs.push("warn:" + m), debug: () => {} };
}
// the verdict lines of a log: the first line, and from the verdict on (the reference's progress lines in between are not reproduced by the wrapper)
const VERDICTS = ["info:PROOF VERIFIED SUCCESSFULLY", "warn:Invalid Proof", "error:Public inputs are not valid.", "error:Proof commitments are not valid",
                  "error:Number of public signals does not match with vk", "error:Proof evaluations are not valid."];
function verdictLines(msgs) {
    const at = msgs.findIndex((m) => VERDICTS.includes(m));
    return at < 0 ? ["no verdict line: " + JSON.stringify(msgs)] : [msgs[0]].concat(msgs.slice(at));
}

async function main() {
    const sets = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
    const origVerify = snarkjs.fflonk.verify, origG16 = snarkjs.groth16.verify, origPlonk = snarkjs.plonk.verify;
    const want = [];
    for (const s of sets) {
        const w = [];
        for (const c of s.cases) { const lg = recorder(); w.push({ ok: await origVerify(s.vk, c.publicSignals, c.proof, lg), msgs: verdictLines(lg.msgs) }); }
        want.push(w);
        const key = new VerifyingKey(s.vk, { device: 0 });
        let refused = false;
        try { await require(path.join(ROOT, "snarkjs_amd", "napi", "zkmi_napi.node")).fflonkVerifyAsync(key.handle, new Uint8Array(12 * 48 + 480), new Uint8Array(32 * key.nPublic), key.nPublic, 1); }
        catch (e) { refused = true; }
        check(s.name + " addon refuses a record buffer of another size", refused);
        const byCount = new Map();
        s.cases.forEach((c, i) => { const k = c.publicSignals.length; if (!byCount.has(k)) byCount.set(k, []); byCount.get(k).push(i); });
        for (const idx of byCount.values()) {
            const got = await key.verifyMany(idx.map((i) => s.cases[i].publicSignals), idx.map((i) => s.cases[i].proof));
            idx.forEach((i, j) => check(s.name + " verifyMany " + s.cases[i].label, got[j] === w[i].ok, "got " + got[j] + " want " + w[i].ok));
        }
        key.release();
    }
    // 3: verify: true alone is Groth16 only
    await registerAll(snarkjs, { fused: true, verify: true });
    check("verify: true keeps the reference's fflonk.verify", snarkjs.fflonk.verify === origVerify && snarkjs.plonk.verify === origPlonk && snarkjs.groth16.verify !== origG16);
    await uninstallFused(snarkjs);
    await registerAll(snarkjs, { fused: true, verify: { groth16: true, plonk: true } });
    check("verify: {groth16, plonk} keeps the reference's fflonk.verify", snarkjs.fflonk.verify === origVerify && snarkjs.plonk.verify !== origPlonk && snarkjs.groth16.verify !== origG16);
    await uninstallFused(snarkjs);
    await registerAll(snarkjs, { fused: true, verifyFflonk: true });
    check("verifyFflonk: true replaces fflonk.verify alone", snarkjs.fflonk.verify !== origVerify && snarkjs.groth16.verify === origG16 && snarkjs.plonk.verify === origPlonk);
    await uninstallFused(snarkjs);
    // 2: the drop-in
    const out = await registerAll(snarkjs, { fused: true, verify: { fflonk: true } });
    check("verify: {fflonk} replaces fflonk.verify alone", snarkjs.fflonk.verify !== origVerify && snarkjs.groth16.verify === origG16 && snarkjs.plonk.verify === origPlonk);
    for (let si = 0; si < sets.length; si++) {
        const s = sets[si], calls = [], loggers = [], idx = [];
        for (let i = 0; i < 128; i++) {
            const k = i % s.cases.length, lg = recorder();
            idx.push(k); loggers.push(lg);
            calls.push(snarkjs.fflonk.verify(s.vk, s.cases[k].publicSignals, s.cases[k].proof, lg));
        }
        const before = out.fused.fflonkVerifier.stats.batches;
        const res = await Promise.all(calls);
        const batches = out.fused.fflonkVerifier.stats.batches - before;
        check(s.name + " 128 concurrent calls: reference results", res.every((r, i) => r === want[si][idx[i]].ok));
        const badLog = loggers.findIndex((lg, i) => JSON.stringify(lg.msgs) !== JSON.stringify(want[si][idx[i]].msgs));
        check(s.name + " 128 concurrent calls: reference verdict messages", badLog < 0,
              badLog < 0 ? "" : s.cases[idx[badLog]].label + " " + JSON.stringify(loggers[badLog].msgs) + " vs " + JSON.stringify(want[si][idx[badLog]].msgs));
        check(s.name + " coalesced into " + batches + " device batches (< 128)", batches >= 1 && batches < 128);
        check(s.name + " without a logger", (await snarkjs.fflonk.verify(s.vk, s.cases[0].publicSignals, s.cases[0].proof)) === want[si][0].ok);
    }
    await uninstallFused(snarkjs);
    check("uninstallFused restores the reference's verify", snarkjs.fflonk.verify === origVerify && snarkjs.groth16.verify === origG16);
    for (const name of ["bn128", "bls12381"]) unregister(await snarkjs.curves.getCurveFromName(name));
    console.log(fails ? "FAILED " + fails : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.log("FAIL exception", e && e.stack || e); process.exit(2); });
