// tests/js/bellman_cpu.js — js/groth16_bellman_native.js without a device (tests/test_node_bellman.py): its parsing, hashing and the bytes it writes against the
// reference's LIVE zKey.exportBellman / bellmanContribute / importBellman under the same pinned getRandomValues stream, with the reference's own curve object
// (G1.fft, G1.ifft, G1.batchApplyKey, G.batchLEMtoU, G.batchUtoLEM) in place of the device calls; the library's host-only calls (the key pair, hashToG2, one
// point times a scalar) are the real ones. Per curve and circuit:
//   1  export -> bellmanContribute -> importBellman through the installed functions (registerAll's installer with this dev): at every step the reference's bytes,
//      returned value and logger lines, and the committed golden file and hashes; one device call per section
//   2  what the reference refuses, as tests/golden/bellman_golden.json records it: its thrown message (a PLONK key), or false with its logger.error line
//      (fewer contributions, a changed old contribution, a wrong count), all before any device work
//   3  the hand-over cases: a parameter file or a challenge cut short, a file that is no zkey, a section 10 cut short, an empty entropy and an unknown curve
//      reach the saved reference function and give its outcome
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/bellman_cpu.js
"use strict";
const fs = require("fs"), path = require("path"), crypto = require("crypto");
const L = require("./ptau_verify_lib.js");
process.env.NTHREADS = process.env.NTHREADS || "8";
const snarkjs = require(path.join(L.ROOT, "oracle", "ref_shim.js"));
const bN = require(path.join(L.ROOT, "snarkjs_amd", "js", "groth16_bellman_native.js"));
const { installBellman, uninstallBellman } = require(path.join(L.ROOT, "snarkjs_amd", "js", "register.js"));
const addon = require(path.join(L.ROOT, "snarkjs_amd", "napi", "zkmi_napi.node"));
const GOLD = JSON.parse(fs.readFileSync(path.join(L.ROOT, "tests", "golden", "bellman_golden.json")));
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }
const same = (a, b) => a.byteLength === b.byteLength && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;
const bytes = (m) => { const d = m.data; return (d instanceof Uint8Array) ? d : d.slice(0, d.byteLength); };
const hex = (b) => (b === undefined || b === null || typeof b === "boolean" ? String(b) : Buffer.from(b).toString("hex"));
const sha = (b) => crypto.createHash("sha256").update(b).digest("hex");
const KEYS = ["exportBellman", "bellmanContribute", "importBellman"];
const m = (d) => ({ type: "mem", data: new Uint8Array(d) });

function refDevice(curve) {
    const calls = [], flat = (r) => (r instanceof Uint8Array ? r : r.slice(0, r.byteLength));
    const G = (group) => (group == 1 ? curve.G1 : curve.G2), Fr = curve.Fr, sG1 = curve.G1.F.n8 * 2;
    return Object.assign(bN.deviceOf(addon), { calls,
        async convert(_cv, group, kind, body) {
            calls.push(["convert", group, kind, body.byteLength]);
            if (!body.byteLength) return new Uint8Array(0);
            return flat(await (kind == 0 ? G(group).batchLEMtoU(Uint8Array.from(body)) : G(group).batchUtoLEM(Uint8Array.from(body))));
        },
        async hSection(_cv, body, power, direction) {
            calls.push(["h", power, direction]);
            if (direction == 0) {
                let t = flat(await curve.G1.fft(Uint8Array.from(body), "affine", "jacobian"));
                t = flat(await curve.G1.batchApplyKey(t, Fr.neg(Fr.e(2)), Fr.w[power + 1], "jacobian", "affine"));
                return flat(await curve.G1.batchLEMtoU(t.slice(0, t.byteLength - sG1)));
            }
            const lem = flat(await curve.G1.batchUtoLEM(Uint8Array.from(body))), h = new Uint8Array(lem.byteLength + sG1);
            h.set(lem);
            const t = flat(await curve.G1.batchApplyKey(h, Fr.neg(Fr.inv(Fr.e(2))), Fr.inv(Fr.w[power + 1]), "affine", "jacobian"));
            return flat(await curve.G1.ifft(t, "jacobian", "affine"));
        },
        async scaleU(_cv, bodyU, k) {
            calls.push(["scale", bodyU.byteLength]);
            if (!bodyU.byteLength) return new Uint8Array(0);
            const lem = flat(await curve.G1.batchUtoLEM(Uint8Array.from(bodyU)));
            return flat(await curve.G1.batchLEMtoU(flat(await curve.G1.batchApplyKey(lem, Uint8Array.from(k), Fr.e(1)))));
        } });
}
function recorder() {
    const lines = [], push = (level) => (text) => lines.push([level, text]);
    return { lines, logger: { debug: () => {}, log: push("log"), info: push("info"), warn: push("warn"), error: push("error") } };
}
// one call of snarkjs.zKey (whatever is installed): { ret, data, lines } or { error, data, lines }
async function call(f) {
    const out = { type: "mem" }, rec = recorder();
    try {
        const ret = await f(out, rec.logger);
        return { ret, data: out.data ? bytes(out) : null, lines: rec.lines };
    } catch (e) { return { error: e.message, data: out.data ? bytes(out) : null, lines: rec.lines }; }
}
async function trip(curve, key, entropy, name) {
    const Z = snarkjs.zKey;
    snarkjs.reseed();
    const ch = await call((o, lg) => Z.exportBellman(m(key), o, lg));
    const rs = await call((o, lg) => Z.bellmanContribute(curve, m(ch.data), o, entropy, lg));
    const nw = await call((o, lg) => Z.importBellman(m(key), m(rs.data), o, name, lg));
    return { ch, rs, nw };
}
// a refused call is compared by its error, returned value and lines (the reference leaves a new file it never closed)
const sameCall = (a, b) => a.error === b.error && hex(a.ret) === hex(b.ret) && L.sameLines(a.lines, b.lines) &&
    (a.error !== undefined || a.ret === false || (b.data !== null && a.data !== null && same(a.data, b.data)));

async function main() {
    const orig = {};
    for (const k of KEYS) orig[k] = snarkjs.zKey[k];
    for (const name of ["bn128", "bls12381"]) {
        const curve = await snarkjs.curves.getCurveFromName(name), dev = refDevice(curve);
        let last = null;
        for (const circuit of ["full", "edge"]) {
            const key = L.G(`phase2_${name}_${circuit}_c1.zkey`), g = GOLD.files[`bellman_${name}_${circuit}_response.params`], imp = GOLD.imported[`${name}_${circuit}`];
            const live = await trip(curve, key, g.entropy, imp.name);
            installBellman(snarkjs, { addon: { init() {} }, dev });
            check(`${name} ${circuit}: the three functions are replaced`, KEYS.every((k) => snarkjs.zKey[k] !== orig[k]));
            const n0 = dev.calls.length, here = await trip(curve, key, g.entropy, imp.name);
            uninstallBellman(snarkjs);
            check(`${name} ${circuit}: uninstall restores the reference's functions`, KEYS.every((k) => snarkjs.zKey[k] === orig[k]));
            for (const [k, label] of [["ch", "exportBellman"], ["rs", "bellmanContribute"], ["nw", "importBellman"]])
                check(`${name} ${circuit}: ${label}: the reference's bytes, returned value and lines`, here[k].error === undefined && sameCall(here[k], live[k]), JSON.stringify([here[k].error, live[k].error, hex(here[k].ret).slice(0, 16), hex(live[k].ret).slice(0, 16)]));
            check(`${name} ${circuit}: the returned values`, here.ch.ret === undefined && here.nw.ret === true && here.rs.lines.length === 1 && here.rs.lines[0][0] === "info" && here.rs.lines[0][1].startsWith("Contribution Hash: "));
            check(`${name} ${circuit}: the committed challenge`, same(here.ch.data, L.G(`bellman_${name}_${circuit}_challenge.params`)));
            check(`${name} ${circuit}: one device call per section`, JSON.stringify(dev.calls.slice(n0).map((c) => c[0])) === JSON.stringify(["convert", "h", "convert", "convert", "convert", "convert", "scale", "scale", "h", "convert"]));
            // the golden response and key were made from the recorded draw: the driver called directly with it
            const direct = await bN.bellmanContribute(name, L.G(g.from), g.entropy, { dev, random64: Buffer.from(g.random64, "hex") });
            check(`${name} ${circuit}: bellmanContribute with the recorded random64: the golden file and hash`, same(direct.response, L.G(`bellman_${name}_${circuit}_response.params`)) && hex(direct.contributionHash) === g.contributionHash);
            const viaCurve = await bN.bellmanContribute(curve, L.G(g.from), g.entropy, { dev, random64: Buffer.from(g.random64, "hex") });
            check(`${name} ${circuit}: the curve object in place of its name`, same(viaCurve.response, direct.response));
            const key2 = await bN.importBellman(key, direct.response, imp.name, { dev });
            check(`${name} ${circuit}: importBellman of it: the recorded key`, sha(key2.zkey) === imp.sha256 && key2.zkey.length === imp.bytes);
            last = { key, here, rs: direct.response };
        }
        // ---- what the reference refuses, and what is handed over (on the edge circuit's files; the PLONK key and the longer key as recorded)
        const Z = () => snarkjs.zKey, { key, rs } = last, R = GOLD.refusals[name];
        const full = L.G(`bellman_${name}_full_response.params`), fullKey = L.G(`phase2_${name}_full_c1.zkey`);
        const flipped = Buffer.from(full), wrongH = Buffer.from(full);
        flipped[R.flipped_transcript.at] ^= 1;
        wrongH.writeUInt32BE(R.wrong_h_count.value, R.wrong_h_count.at);
        const cases = [
            ["plonk_export", false, (o, lg) => Z().exportBellman(m(L.G("plonk_bn128_small.zkey")), o, lg)],
            ["plonk_import", false, (o, lg) => Z().importBellman(m(L.G("plonk_bn128_small.zkey")), m(full), o, "x", lg)],
            ["fewer_contributions", false, (o, lg) => Z().importBellman(m(L.G(R.fewer_contributions.old)), m(full), o, "x", lg)],
            ["flipped_transcript", false, (o, lg) => Z().importBellman(m(fullKey), m(flipped), o, "x", lg)],
            ["wrong_h_count", false, (o, lg) => Z().importBellman(m(fullKey), m(wrongH), o, "x", lg)],
            ["cut_by_10", true, (o, lg) => Z().importBellman(m(fullKey), m(full.subarray(0, full.length - 10)), o, "x", lg)],
            ["a challenge cut short", true, (o, lg) => Z().bellmanContribute(curve, m(rs.subarray(0, rs.length - 10)), o, "e", lg)],
            ["export from a file that is no zkey", true, (o, lg) => Z().exportBellman(m(L.G(`setup_${name}_p8.ptau`)), o, lg)],
            ["import onto a key with section 10 cut short", true, (o, lg) => Z().importBellman(m(L.join(key, L.split(key).map(([t, b]) => [t, t == 10 ? b.subarray(0, b.length - 9) : b]))), m(rs), o, "x", lg)],
        ];
        for (const [label, handed, f] of cases) {
            const ref = await call(f);
            installBellman(snarkjs, { addon: { init() {} }, dev });
            const n0 = dev.calls.length, inst = await call(f);
            uninstallBellman(snarkjs);
            const rec = R[label];
            check(`${name}: ${label}: the reference's outcome (${ref.error || ref.ret})`, (ref.error !== undefined || ref.ret === false) && sameCall(inst, ref) &&
                  (!rec || (rec.threw === inst.error && (rec.returned === undefined || rec.returned === inst.ret) && L.sameLines(inst.lines, rec.lines))), JSON.stringify([inst.error, ref.error, inst.ret, ref.ret, inst.lines, ref.lines]));
            check(`${name}: ${label}: ${handed ? "handed over before" : "refused before"} any device work`, dev.calls.length === n0);
        }
        // the driver itself marks the hand-offs
        for (const [label, f] of [["a parameter file cut short", () => bN.importBellman(fullKey, full.subarray(0, full.length - 10), "x", { dev })], ["a file that is no zkey", () => bN.exportBellman(L.G(`setup_${name}_p8.ptau`), { dev })],
                                  ["an empty entropy", () => bN.bellmanContribute(name, rs, "", { dev })], ["an unknown curve", () => bN.bellmanContribute("secp256k1", rs, "e", { dev })]]) {
            let handed = false;
            try { await f(); } catch (e) { handed = e instanceof bN.BellmanRefusal && e.handOver === true; }
            check(`${name}: ${label}: BellmanRefusal with handOver`, handed);
        }
        // an empty entropy through the installed function reaches the saved one
        installBellman(snarkjs, { addon: { init() {} }, dev });
        const seen = [], savedFn = snarkjs.__zkmiBellman.saved.bellmanContribute;
        uninstallBellman(snarkjs);
        snarkjs.zKey = Object.freeze(Object.assign({}, snarkjs.zKey, { bellmanContribute: async (...a) => { seen.push(a[3]); return "saved"; } }));
        installBellman(snarkjs, { addon: { init() {} }, dev });
        const got = await snarkjs.zKey.bellmanContribute(curve, m(rs), { type: "mem" }, "", null);
        uninstallBellman(snarkjs);
        snarkjs.zKey = Object.freeze(Object.assign({}, snarkjs.zKey, { bellmanContribute: savedFn }));
        check(`${name}: an empty entropy reaches the saved function`, got === "saved" && seen.length === 1 && seen[0] === "" && snarkjs.zKey.bellmanContribute === orig.bellmanContribute);
    }
    console.log(fails ? `${fails} FAILED` : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.error(e); process.exit(1); });
