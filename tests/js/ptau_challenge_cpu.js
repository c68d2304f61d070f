// tests/js/ptau_challenge_cpu.js — js/powersoftau_challenge_native.js without a device (tests/test_node_ptau_challenge.py): its parsing, hashing and the bytes it
// writes against the reference's LIVE powersOfTau.exportChallenge / challengeContribute / importResponse under the same pinned getRandomValues stream, with the
// reference's own curve object (G.batchUtoLEM, G.batchApplyKey, G.batchLEMtoC, G.batchCtoLEM, G.batchLEMtoU) in place of the device calls; the library's host-only
// calls (the key pair, hashToG2, one point times a scalar, the hasher state) are the real ones. Per curve:
//   1  at power 1 and at power 5, from the committed c1 file: export -> challengeContribute -> importResponse with and without points, through the installed
//      functions (registerAll's installer with this dev): at every step the reference's bytes and returned value, the committed golden file, the logger's lines
//   2  the reference's own powersOfTau.verify accepts the file imported by the driver; a second response imports onto both imports as the reference has it
//   3  what the reference refuses: its thrown message and lines; a Groth16 zkey, a file without section 1, a section 7 cut short, power 0 in importResponse, an
//      empty entropy: the driver hands the call over and the installed function gives what the saved function gives
//   4  the cut list of the response hasher where a second chunk appears
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/ptau_challenge_cpu.js
"use strict";
const path = require("path");
const L = require("./ptau_verify_lib.js");
process.env.NTHREADS = process.env.NTHREADS || "8";
const snarkjs = require(path.join(L.ROOT, "oracle", "ref_shim.js"));
const chN = require(path.join(L.ROOT, "snarkjs_amd", "js", "powersoftau_challenge_native.js"));
const setupN = require(path.join(L.ROOT, "snarkjs_amd", "js", "groth16_setup_native.js"));
const { installPtauChallenge, uninstallPtauChallenge } = require(path.join(L.ROOT, "snarkjs_amd", "js", "register.js"));
const addon = require(path.join(L.ROOT, "snarkjs_amd", "napi", "zkmi_napi.node"));
const GOLD = JSON.parse(require("fs").readFileSync(path.join(L.ROOT, "tests", "golden", "ptau_challenge_golden.json")));
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }
const same = (a, b) => a.byteLength === b.byteLength && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;
const bytes = (m) => { const d = m.data; return (d instanceof Uint8Array) ? d : d.slice(0, d.byteLength); };
const hex = (b) => (b === undefined || b === null ? String(b) : Buffer.from(b).toString("hex"));
const KEYS = ["exportChallenge", "challengeContribute", "importResponse"];
const m = (d) => ({ type: "mem", data: new Uint8Array(d) });
L.subtleShim();

function refDevice(curve) {
    const calls = [], flat = (r) => (r instanceof Uint8Array ? r : r.slice(0, r.byteLength));
    const G = (group) => (group == 1 ? curve.G1 : curve.G2);
    return Object.assign(chN.deviceOf(addon), { calls,
        async convert(_cv, group, kind, body, n) { calls.push(["convert", group, n]); return flat(await (kind == 0 ? G(group).batchLEMtoU(Uint8Array.from(body)) : G(group).batchCtoLEM(Uint8Array.from(body)))); },
        async challengeSection(_cv, group, bodyU, n, first, inc) {
            calls.push(["challenge", group, n]);
            const lem = flat(await G(group).batchUtoLEM(Uint8Array.from(bodyU)));
            return flat(await G(group).batchLEMtoC(flat(await G(group).batchApplyKey(lem, Uint8Array.from(first), Uint8Array.from(inc)))));
        },
        async importSection(_cv, group, bodyC, n) {
            calls.push(["import", group, n]);
            const lem = flat(await G(group).batchCtoLEM(Uint8Array.from(bodyC)));
            return { lem, u: flat(await G(group).batchLEMtoU(lem)) };
        } });
}
function recorder() {
    const lines = [], push = (level) => (text) => lines.push([level, text]);
    return { lines, logger: { debug: () => {}, log: push("log"), info: push("info"), warn: push("warn"), error: push("error") } };
}
// one call of snarkjs.powersOfTau (whatever is installed): { ret, data, lines } or { error, data, lines }
async function call(f) {
    const out = { type: "mem" }, rec = recorder();
    try {
        const ret = await f(out, rec.logger);
        return { ret, data: out.data ? bytes(out) : null, lines: rec.lines };
    } catch (e) { return { error: e.message, data: out.data ? bytes(out) : null, lines: rec.lines }; }
}
// the round trip from `old` through whatever is installed, under the pinned stream
async function trip(curve, old, entropy, name) {
    const P = snarkjs.powersOfTau;
    snarkjs.reseed();
    const ch = await call((o, lg) => P.exportChallenge(m(old), o, lg));
    const rs = await call((o, lg) => P.challengeContribute(curve, m(ch.data), o, entropy, lg));
    const full = await call((o, lg) => P.importResponse(m(old), m(rs.data), o, name, true, lg));
    const bare = await call((o, lg) => P.importResponse(m(old), m(rs.data), o, name, false, lg));
    return { ch, rs, full, bare };
}
// a call that throws is compared by its error and lines (the reference leaves a new file it never closed)
const sameCall = (a, b) => a.error === b.error && hex(a.ret) === hex(b.ret) && L.sameLines(a.lines, b.lines) && (a.error !== undefined || (b.data !== null && a.data !== null && same(a.data, b.data)));

async function main() {
    const orig = {};
    for (const k of KEYS) orig[k] = snarkjs.powersOfTau[k];
    for (const name of ["bn128", "bls12381"]) {
        const curve = await snarkjs.curves.getCurveFromName(name), cv = setupN.CURVES.find((c) => c.name === name);
        const dev = refDevice(curve);
        let last = null;
        for (const power of [1, 5]) {
            const g = GOLD.trips[`${name}_p${power}`], old = L.G(g.from);
            const live = await trip(curve, old, g.entropy, g.name);
            installPtauChallenge(snarkjs, { addon: { init() {} }, dev });
            check(`${name} p${power}: the three functions are replaced`, KEYS.every((k) => snarkjs.powersOfTau[k] !== orig[k]));
            const n0 = dev.calls.length, here = await trip(curve, old, g.entropy, g.name);
            uninstallPtauChallenge(snarkjs);
            check(`${name} p${power}: uninstall restores the reference's functions`, KEYS.every((k) => snarkjs.powersOfTau[k] === orig[k]));
            for (const [k, label, file] of [["ch", "exportChallenge", "challenge"], ["rs", "challengeContribute", "response"], ["full", "importResponse", "imported"], ["bare", "importResponse without points", "nopoints"]]) {
                check(`${name} p${power}: ${label}: the reference's bytes, returned value and lines`, sameCall(here[k], live[k]), JSON.stringify([here[k].error, live[k].error]));
                check(`${name} p${power}: ${label}: the committed golden file`, here[k].data !== null && same(here[k].data, L.G(g.files[file].file)));
            }
            check(`${name} p${power}: the recorded hashes and lines`, hex(here.ch.ret) === g.challengeHash && hex(here.full.ret) === g.nextChallenge && hex(here.bare.ret) === g.noPointsReturned &&
                  here.rs.ret === undefined && L.sameLines(here.ch.lines, g.lines.exportChallenge) && L.sameLines(here.rs.lines, g.lines.challengeContribute) &&
                  L.sameLines(here.full.lines, g.lines.importResponse) && L.sameLines(here.bare.lines, g.lines.importResponseNoPoints));
            const n = 2 ** power, want = [["convert", 1, 2 * n - 1], ["convert", 2, n], ["convert", 1, n], ["convert", 1, n], ["convert", 2, 1], ["challenge", 1, 2 * n - 1], ["challenge", 2, n],
                                         ["challenge", 1, n], ["challenge", 1, n], ["challenge", 2, 1], ["import", 1, 2 * n - 1], ["import", 2, n], ["import", 1, n], ["import", 1, n], ["import", 2, 1]];
            check(`${name} p${power}: one device call per section`, JSON.stringify(dev.calls.slice(n0, n0 + 15)) === JSON.stringify(want) && dev.calls.length === n0 + 20);
            check(`${name} p${power}: the reference's verify accepts the file imported here`, (await snarkjs.powersOfTau.verify(m(here.full.data))) === true);
            last = { old, here, g };
        }
        // ---- the driver called directly with the recorded random64, and a second response onto both imports
        const g = last.g;
        const direct = await chN.challengeContribute(name, L.G(g.files.challenge.file), g.entropy, { dev, random64: Buffer.from(g.random64, "hex") });
        check(`${name}: challengeContribute with the recorded random64: the golden file`, same(direct.response, L.G(g.files.response.file)));
        const s = GOLD.second[name];
        const ch2 = await chN.exportChallenge(last.here.full.data, { dev });
        const rs2 = await chN.challengeContribute(name, ch2.challenge, s.entropy, { dev, random64: Buffer.from(s.random64, "hex") });
        const sha = (b) => require("crypto").createHash("sha256").update(b).digest("hex");
        const onto = [await chN.importResponse(last.here.full.data, rs2.response, s.name, true, { dev }), await chN.importResponse(last.here.bare.data, rs2.response, s.name, true, { dev })];
        check(`${name}: a second response onto the import with points and onto the one without: the reference's file`, sha(rs2.response) === s.responseSha256 &&
              sha(onto[0].ptau) === s.ontoFull.sha256 && sha(onto[1].ptau) === s.ontoNoPoints.sha256 && hex(onto[1].nextChallenge) === s.ontoNoPoints.returns);
        // ---- what the reference refuses, and what is handed over
        const P = () => snarkjs.powersOfTau, h = last.here, old = last.old;
        const secs = L.split(old), s1 = 2 * cv.n8q;
        const broken = L.join(old, secs.map(([t, b]) => [t, t == 2 ? new Uint8Array(Buffer.concat([Buffer.from(b.subarray(s1, 2 * s1)), Buffer.from(b.subarray(s1))])) : b]));
        const plus = (b) => new Uint8Array(Buffer.concat([Buffer.from(b), Buffer.alloc(1)]));
        const p0 = bytes(await (async () => { const f = { type: "mem" }; await snarkjs.powersOfTau.newAccumulator(curve, 0, f); return f; })());
        const ch0 = await chN.exportChallenge(p0, { dev }), rs0 = await chN.challengeContribute(name, ch0.challenge, "e", { dev, random64: Buffer.alloc(64) });
        const cases = [
            ["export from a file imported without points", false, (o, lg) => P().exportChallenge(m(h.bare.data), o, lg)],
            ["export from a file whose points are not the declared ones", false, (o, lg) => P().exportChallenge(m(broken), o, lg)],
            ["a challenge one byte longer", false, (o, lg) => P().challengeContribute(curve, m(plus(h.ch.data)), o, "e", lg)],
            ["a challenge one byte shorter", false, (o, lg) => P().challengeContribute(curve, m(h.ch.data.subarray(0, h.ch.data.length - 1)), o, "e", lg)],
            ["a response one byte longer", false, (o, lg) => P().importResponse(m(old), m(plus(h.rs.data)), o, "x", true, lg)],
            ["a response of another power", false, (o, lg) => P().importResponse(m(L.G(`ptau_${name}_p1_c1.ptau`)), m(h.rs.data), o, "x", true, lg)],
            ["a response to another challenge", false, (o, lg) => P().importResponse(m(h.full.data), m(h.rs.data), o, "x", true, lg)],
            ["export from a Groth16 zkey", true, (o, lg) => P().exportChallenge(m(L.G(`groth16_${name}_n1024.zkey`)), o, lg)],
            ["export from a file without section 1", true, (o, lg) => P().exportChallenge(m(L.join(old, secs.filter(([t]) => t != 1))), o, lg)],
            ["export with section 7 cut short", true, (o, lg) => P().exportChallenge(m(L.join(old, secs.map(([t, b]) => [t, t == 7 ? b.subarray(0, b.length - 9) : b]))), o, lg)],
            ["import with section 7 cut short", true, (o, lg) => P().importResponse(m(L.join(old, secs.map(([t, b]) => [t, t == 7 ? b.subarray(0, b.length - 9) : b]))), m(h.rs.data), o, "x", true, lg)],
            ["import at power 0", true, (o, lg) => P().importResponse(m(p0), m(rs0.response), o, "C1", true, lg)],
            ["import at power 0 without points", true, (o, lg) => P().importResponse(m(p0), m(rs0.response), o, "C1", false, lg)],
        ];
        for (const [label, handed, f] of cases) {
            const ref = await call(f);
            installPtauChallenge(snarkjs, { addon: { init() {} }, dev });
            const n0 = dev.calls.length, inst = await call(f);
            uninstallPtauChallenge(snarkjs);
            const rec = GOLD.refused.find((x) => x.curve === name && x.label === label);
            check(`${name}: ${label}: the reference's outcome (${ref.error})`, ref.error !== undefined && sameCall(inst, ref) && (!rec || (rec.throws === inst.error && L.sameLines(inst.lines, rec.lines))),
                  JSON.stringify([inst.error, ref.error, inst.lines.length, ref.lines.length]));
            if (label === "export from a file whose points are not the declared ones") check(`${name}: ${label}: the challenge is written all the same, as the reference writes it`, inst.data !== null && same(inst.data, ref.data));
            if (handed) check(`${name}: ${label}: handed over before any device work`, dev.calls.length === n0);
        }
        // the driver itself marks the hand-offs
        for (const [label, f] of [["a Groth16 zkey", () => chN.exportChallenge(L.G(`groth16_${name}_n1024.zkey`), { dev })], ["power 0", () => chN.importResponse(p0, rs0.response, "C1", true, { dev })],
                                  ["an empty entropy", () => chN.challengeContribute(name, h.ch.data, "", { dev })], ["an unknown curve", () => chN.challengeContribute("secp256k1", h.ch.data, "e", { dev })]]) {
            let handed = false;
            try { await f(); } catch (e) { handed = e instanceof chN.ChallengeRefusal && e.handOver === true; }
            check(`${name}: ${label}: ChallengeRefusal with handOver`, handed);
        }
    }
    // ---- the cut list (BN254 powers 17 - 19, BLS12-381 powers 16 - 18; tests/test_ptau_challenge_host.py holds the Python twin to the same numbers)
    const bn = setupN.CURVES.find((c) => c.name === "bn128"), bls = setupN.CURVES.find((c) => c.name === "bls12381"), M = 1 << 20;
    const eq = (a, b) => JSON.stringify(a) === JSON.stringify(b);
    const g1 = Math.floor(2 ** 24 / 96), g2 = Math.floor(2 ** 24 / 192), h1 = Math.floor(2 ** 24 / 48), h2 = Math.floor(2 ** 24 / 96);
    check("responseCuts: BN254", eq(chN.responseCuts(bn, 17, true), [64, (2 ** 18 - 1) * 32, 8 * M, 4 * M, 4 * M, 64]) &&
          eq(chN.responseCuts(bn, 18, true), [64, 8 * M, (2 ** 18 - 1) * 32, 8 * M, 8 * M, 8 * M, 8 * M, 64]) && eq(chN.responseCuts(bn, 18, false), [64, (2 ** 19 - 1) * 32, 16 * M, 8 * M, 8 * M, 64]) &&
          eq(chN.responseCuts(bn, 19, false), [64, 16 * M, (2 ** 19 - 1) * 32, 16 * M, 16 * M, 16 * M, 16 * M, 64]));
    check("responseCuts: BLS12-381", eq(chN.responseCuts(bls, 16, true), [64, (2 ** 17 - 1) * 48, 2 ** 16 * 96, 2 ** 16 * 48, 2 ** 16 * 48, 96]) &&
          eq(chN.responseCuts(bls, 17, true), [64, g1 * 48, (2 ** 18 - 1 - g1) * 48, g2 * 96, (2 ** 17 - g2) * 96, 2 ** 17 * 48, 2 ** 17 * 48, 96]) &&
          eq(chN.responseCuts(bls, 17, false), [64, (2 ** 18 - 1) * 48, 2 ** 17 * 96, 2 ** 17 * 48, 2 ** 17 * 48, 96]) &&
          eq(chN.responseCuts(bls, 18, false), [64, h1 * 48, (2 ** 19 - 1 - h1) * 48, h2 * 96, (2 ** 18 - h2) * 96, 2 ** 18 * 48, 2 ** 18 * 48, 96]));
    console.log(fails ? `${fails} FAILED` : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.error(e); process.exit(1); });
