// tests/js/wtns_check_gpu.js — snarkjs.wtns.check on the device through the real addon (tests/test_node_wtns_check.py). In ONE process, every case of
// tests/golden/wtns_check_golden.json runs unpatched and under registerAll(snarkjs, { wtnsCheck: true }):
//   1  registerAll(snarkjs) leaves wtns.check the reference's; { wtnsCheck: true } replaces it
//   2  every case: the reference's verdict or thrown message and its lines, with a logger and without one (where the reference reads beyond a buffer its own
//      answer comes from stale memory: there the replacement hands the call over, and only a thrown message is compared)
//   3  the addon's r1csLoad / r1csCheck on a batch of witnesses; unregister restores the reference's function
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/wtns_check_gpu.js
"use strict";
const fs = require("fs"), path = require("path");
const ROOT = path.join(__dirname, "..", "..");
process.env.NTHREADS = process.env.NTHREADS || "8";
const snarkjs = require(path.join(ROOT, "oracle", "ref_shim.js"));
const { registerAll, unregister, loadAddon } = require(path.join(ROOT, "snarkjs_amd", "js", "register.js"));
const wtnsN = require(path.join(ROOT, "snarkjs_amd", "js", "wtns_check_native.js"));
const GOLD = path.join(ROOT, "tests", "golden");
const CASES = JSON.parse(fs.readFileSync(path.join(GOLD, "wtns_check_golden.json"))).cases;
const G = (f) => new Uint8Array(fs.readFileSync(path.join(GOLD, f)));
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }
function recorder() {
    const lines = [], push = (level) => (text) => lines.push([level, text]);
    return { lines, logger: { debug: push("debug"), log: push("log"), info: push("info"), warn: push("warn"), error: push("error") } };
}
async function capture(f, withLogger) {
    const rec = recorder();
    try { return { returns: await f(withLogger ? rec.logger : undefined), lines: rec.lines }; } catch (e) { return { throws: e.message, lines: rec.lines }; }
}
const sameLines = (a, b) => JSON.stringify(a) === JSON.stringify(b);

async function main() {
    const orig = snarkjs.wtns.check;
    const ref = {};
    for (const c of CASES) ref[c.name] = [await capture((lg) => orig(G(c.r1cs), G(c.wtns), lg), true), await capture((lg) => orig(G(c.r1cs), G(c.wtns), lg), false)];
    await registerAll(snarkjs);
    check("registerAll(snarkjs) keeps the reference's wtns.check", snarkjs.wtns.check === orig);
    await registerAll(snarkjs, { wtnsCheck: true });
    check("{ wtnsCheck: true } replaces it", snarkjs.wtns.check !== orig);
    for (const c of CASES) {
        for (const withLogger of [true, false]) {
            const label = `${c.name}${withLogger ? "" : " (no logger)"}`, want = ref[c.name][withLogger ? 0 : 1];
            const got = await capture((lg) => snarkjs.wtns.check(G(c.r1cs), G(c.wtns), lg), withLogger);
            if (c.readsPast) { if (want.throws !== undefined) check(`${label}: the reference's thrown message`, got.throws === want.throws, JSON.stringify([got.throws, want.throws])); continue; }
            check(`${label}: the reference's verdict or thrown message`, got.returns === want.returns && got.throws === want.throws, JSON.stringify([got.returns, got.throws, want.returns, want.throws]));
            check(`${label}: the reference's lines`, sameLines(got.lines, want.lines), JSON.stringify(got.lines) + " / " + JSON.stringify(want.lines));
            check(`${label}: the recorded answer`, got.returns === (withLogger ? c : c.noLogger).returns && got.throws === (withLogger ? c : c.noLogger).throws);
        }
    }
    // the addon's two entries on a batch
    const addon = loadAddon(), dev = wtnsN.deviceOf(addon), by = Object.fromEntries(CASES.map((c) => [c.name, c]));
    for (const name of ["bn128", "bls12381"]) {
        const inp = wtnsN.readInputs(G(by[`${name}_good`].r1cs), G(by[`${name}_good`].wtns));
        const ws = ["good", "bad_two", "bad_last", "wide_witness", "bad_first"].map((n) => wtnsN.readInputs(G(by[`${name}_${n}`].r1cs), G(by[`${name}_${n}`].wtns)).witness);
        const key = dev.load(inp.cv, inp.constraints, inp.head.nConstraints, inp.head.nVars);
        const got = dev.check(key, new Uint8Array(Buffer.concat(ws)), ws.length);
        check(`${name}: a batch of five through r1csLoad / r1csCheck`, JSON.stringify(got) === JSON.stringify([wtnsN.NONE, 9, 12, wtnsN.NONE, 0]), JSON.stringify(got));
        let msg = "";
        try { addon.r1csCheck(key, ws[0].subarray(32), 1); } catch (e) { msg = e.message; }
        check(`${name}: a witness of the wrong length is refused`, /witness_len/.test(msg), msg);
        dev.release(key);
        msg = "";
        try { addon.r1csCheck(key, ws[0], 1); } catch (e) { msg = e.message; }
        check(`${name}: released`, /no r1cs is resident/.test(msg), msg);
    }
    unregister(snarkjs);
    check("unregister restores the reference's wtns.check", snarkjs.wtns.check === orig);
    console.log(fails ? `${fails} FAILED` : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.error(e); process.exit(1); });
