// tests/js/ptau_contribute_cpu.js — js/powersoftau_contribute_native.js without a device (tests/test_node_ptau_contribute.py): its parsing, hashing and the bytes
// it writes against the reference's LIVE powersOfTau.newAccumulator / contribute / beacon under the same pinned getRandomValues stream, with the reference's own
// curve object (G.batchApplyKey, G.batchLEMtoC, G.batchLEMtoU) in place of the device call; the library's host-only calls (the key pair, hashToG2, one point
// times a scalar, the hasher state) are the real ones. Per curve:
//   1  a ceremony at power 1 and at power 5, new -> C1 -> C2 -> B3: at every step the reference's bytes and returned hash, the committed golden file, the logger's
//      info lines; through the installed functions (registerAll's installer with this dev) too
//   2  the ceremony made by the driver alone is accepted by the reference's powersOfTau.verify, also after the reference's preparePhase2
//   3  what the reference refuses: its thrown message, or false and its logger lines; power 0, a Groth16 zkey, a file without section 3, an empty section 7 cut
//      short: the driver hands the call over and the installed function gives what the saved function gives
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/ptau_contribute_cpu.js
"use strict";
const path = require("path");
const L = require("./ptau_verify_lib.js");
process.env.NTHREADS = process.env.NTHREADS || "8";
const snarkjs = require(path.join(L.ROOT, "oracle", "ref_shim.js"));
const contribN = require(path.join(L.ROOT, "snarkjs_amd", "js", "powersoftau_contribute_native.js"));
const setupN = require(path.join(L.ROOT, "snarkjs_amd", "js", "groth16_setup_native.js"));
const { installPtauContribute, uninstallPtauContribute } = require(path.join(L.ROOT, "snarkjs_amd", "js", "register.js"));
const addon = require(path.join(L.ROOT, "snarkjs_amd", "napi", "zkmi_napi.node"));
const GOLD = JSON.parse(require("fs").readFileSync(path.join(L.ROOT, "tests", "golden", "ptau_contribute_golden.json")));
const BEACON = Array.from({ length: 31 }, (_, i) => (i + 1).toString(16).padStart(2, "0")).join("");
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }
const same = (a, b) => a.byteLength === b.byteLength && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;
const bytes = (m) => { const d = m.data; return (d instanceof Uint8Array) ? d : d.slice(0, d.byteLength); };
const hex = (b) => Buffer.from(b).toString("hex");
L.subtleShim();

function refDevice(curve, cv) {
    const calls = [], flat = (r) => (r instanceof Uint8Array ? r : r.slice(0, r.byteLength));
    return Object.assign(contribN.deviceOf(addon), { calls,
        async contributeSection(_cv, group, body, n, first, inc) {
            const G = group == 1 ? curve.G1 : curve.G2;
            calls.push([group, n]);
            const lem = flat(await G.batchApplyKey(Uint8Array.from(body), Uint8Array.from(first), Uint8Array.from(inc)));
            return { lem, c: flat(await G.batchLEMtoC(lem)), u: flat(await G.batchLEMtoU(lem)) };
        } });
}
const STEPS = [["c1", "contribute", { name: "C1", entropy: "Entropy1" }], ["c2", "contribute", { name: "C2", entropy: "Entropy2" }],
               ["b3", "beacon", { name: "B3", beaconHash: BEACON, numIterationsExp: 10 }]];
function recorder() {
    const lines = [], push = (level) => (text) => lines.push([level, text]);
    return { lines, logger: { debug: () => {}, log: push("log"), info: push("info"), warn: push("warn"), error: push("error") } };
}
// one call of snarkjs.powersOfTau (whatever is installed): { ret, data, lines } or { error, lines }
async function call(op, old, a) {
    const out = { type: "mem" }, rec = recorder();
    try {
        const ret = op === "contribute" ? await snarkjs.powersOfTau.contribute({ type: "mem", data: old }, out, a.name, a.entropy, rec.logger)
                                        : await snarkjs.powersOfTau.beacon({ type: "mem", data: old }, out, a.name, a.beaconHash, a.numIterationsExp, rec.logger);
        return { ret, data: out.data ? bytes(out) : null, lines: rec.lines };
    } catch (e) { return { error: e.message, lines: rec.lines }; }
}

async function main() {
    for (const name of ["bn128", "bls12381"]) {
        const curve = await snarkjs.curves.getCurveFromName(name), cv = setupN.CURVES.find((c) => c.name === name);
        const dev = refDevice(curve, cv);
        const orig = { newAccumulator: snarkjs.powersOfTau.newAccumulator, contribute: snarkjs.powersOfTau.contribute, beacon: snarkjs.powersOfTau.beacon };
        for (const power of [1, 5]) {
            // ---- the reference, live, under the pinned stream
            snarkjs.reseed();
            const a0 = { type: "mem" }, live = [];
            const first = await snarkjs.powersOfTau.newAccumulator(curve, power, a0);
            let prev = bytes(a0);
            for (const [, op, a] of STEPS) { const r = await call(op, prev, a); live.push(r); prev = r.data; }
            // ---- the installed functions with this dev, under the same stream
            installPtauContribute(snarkjs, { addon: { init() {} }, dev });
            check(`${name} p${power}: the three functions are replaced`, ["newAccumulator", "contribute", "beacon"].every((k) => snarkjs.powersOfTau[k] !== orig[k]));
            snarkjs.reseed();
            const b0 = { type: "mem" }, rec0 = recorder(), n0 = dev.calls.length;
            const first2 = await snarkjs.powersOfTau.newAccumulator(curve, power, b0, rec0.logger);
            const fresh = GOLD.fresh[`${name}_p${power}`];
            check(`${name} p${power}: newAccumulator: the reference's bytes and first challenge hash`, same(bytes(b0), bytes(a0)) && hex(first2) === hex(first) && hex(first) === fresh.firstChallengeHash);
            check(`${name} p${power}: newAccumulator: the info line`, L.sameLines(rec0.lines.filter((x) => x[0] !== "debug"), fresh.lines.filter((x) => x[0] !== "debug")));
            prev = bytes(b0);
            for (let i = 0; i < STEPS.length; i++) {
                const [tag, op, a] = STEPS[i], r = await call(op, prev, a), file = `ptau_${name}_p${power}_${tag}.ptau`;
                check(`${name} p${power}: ${op}(${a.name}): the reference's bytes and returned hash`, r.error === undefined && same(r.data, live[i].data) && hex(r.ret) === hex(live[i].ret), r.error);
                check(`${name} p${power}: ${op}(${a.name}): the committed golden file`, r.error === undefined && same(r.data, L.G(file)) && hex(r.ret) === GOLD.steps[file].returned);
                check(`${name} p${power}: ${op}(${a.name}): the logger's lines`, L.sameLines(r.lines, live[i].lines) && L.sameLines(r.lines, GOLD.steps[file].lines));
                prev = r.data;
            }
            check(`${name} p${power}: one device call per section`, JSON.stringify(dev.calls.slice(n0, n0 + 4)) === JSON.stringify([[1, 2 * 2 ** power - 1], [2, 2 ** power], [1, 2 ** power], [1, 2 ** power]]) &&
                  dev.calls.length === n0 + 12);
            uninstallPtauContribute(snarkjs);
            check(`${name} p${power}: uninstall restores the reference's functions`, ["newAccumulator", "contribute", "beacon"].every((k) => snarkjs.powersOfTau[k] === orig[k]));
            // ---- the ceremony made by the driver alone, accepted by the reference
            const made = prev;
            check(`${name} p${power}: the reference's verify accepts the ceremony made here`, (await snarkjs.powersOfTau.verify({ type: "mem", data: made })) === true);
            if (power == 5) {
                const prepared = { type: "mem" };
                await snarkjs.powersOfTau.preparePhase2({ type: "mem", data: made }, prepared);
                check(`${name} p${power}: and after preparePhase2`, (await snarkjs.powersOfTau.verify({ type: "mem", data: bytes(prepared) })) === true);
            }
        }
        // ---- the driver called directly, with a given random64
        const g = GOLD.steps[`ptau_${name}_p5_c1.ptau`];
        const fresh5 = (await contribN.newAccumulator(name, 5)).ptau;
        const direct = await contribN.contribute(fresh5, g.name, g.entropy, { dev, random64: Buffer.from(g.random64, "hex") });
        check(`${name}: contribute with the recorded random64: the golden file`, same(direct.ptau, L.G(`ptau_${name}_p5_c1.ptau`)) && hex(direct.responseHash) === g.returned);
        // ---- what the reference refuses, and what is handed over
        const c1 = L.G(`ptau_${name}_p5_c1.ptau`);
        installPtauContribute(snarkjs, { addon: { init() {} }, dev });
        for (const c of GOLD.refused.filter((x) => x.curve === name)) {
            let old = c1;
            if (c.rule === "truncate4") { const cutAll = L.caseFile({ fixture: `ptau_${name}_p5_c1.ptau`, rule: "truncate4" }, cv.n8q); old = L.join(cutAll, L.split(cutAll).filter(([t]) => t < 12)); }
            const n0 = dev.calls.length, r = await call(c.op, old, c);
            const want = c.throws !== undefined ? r.error === c.throws : (r.error === undefined && r.ret === false);
            check(`${name}: ${c.label}: as the reference (${c.throws !== undefined ? "throws" : "false"}), its lines, no device call`, want && L.sameLines(r.lines, c.lines) && dev.calls.length === n0,
                  JSON.stringify([r.error, r.ret, r.lines]));
        }
        const secs = L.split(c1);
        const bad = [["a Groth16 zkey", L.G(`groth16_${name}_n1024.zkey`)], ["no section 3", L.join(c1, secs.filter(([t]) => t != 3))],
                     ["section 4 one byte short", L.join(c1, secs.map(([t, b]) => [t, t == 4 ? b.subarray(0, b.length - 1) : b]))],
                     ["section 7 cut short", L.join(c1, secs.map(([t, b]) => [t, t == 7 ? b.subarray(0, b.length - 9) : b]))],
                     ["power 0", bytes(await (async () => { const m = { type: "mem" }; await orig.newAccumulator(curve, 0, m); return m; })())]];
        for (const [what, raw] of bad) for (const [op, a] of [["contribute", { name: "X", entropy: "e" }], ["beacon", { name: "X", beaconHash: BEACON, numIterationsExp: 10 }]]) {
            const n0 = dev.calls.length;
            let handed = false;
            try { await (op === "contribute" ? contribN.contribute(raw, a.name, a.entropy, { dev }) : contribN.beacon(raw, a.name, a.beaconHash, a.numIterationsExp, { dev })); }
            catch (e) { handed = e instanceof contribN.ContributeRefusal && e.handOver === true; }
            check(`${name}: ${op}(${what}): handed over before any device work`, handed && dev.calls.length === n0);
            uninstallPtauContribute(snarkjs);
            snarkjs.reseed();
            const ref = await call(op, raw, a);
            installPtauContribute(snarkjs, { addon: { init() {} }, dev });
            snarkjs.reseed();
            const inst = await call(op, raw, a);
            check(`${name}: ${op}(${what}): the saved function's outcome`, inst.error === ref.error && (ref.error !== undefined || (ref.ret === false ? inst.ret === false : ref.data !== null && inst.data !== null)),
                  JSON.stringify([inst.error, ref.error]));
        }
        uninstallPtauContribute(snarkjs);
    }
    // ---- the hasher state through the addon
    for (const v of GOLD.blake2bPartial.vectors) {
        let at = 0;
        const chunks = v.lens.map((n) => { const d = new Uint8Array(n); for (let i = 0; i < n; i++) d[i] = (7 * (at + i) + 3) & 255; at += n; return d; });
        check(`blake2b512Partial(${v.lens.join(", ")})`, hex(addon.blake2b512Partial(chunks)) === v.partial);
    }
    console.log(fails ? `${fails} FAILED` : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.error(e); process.exit(1); });
