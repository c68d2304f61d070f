// tests/js/ptau_challenge_gpu.js — snarkjs.powersOfTau.exportChallenge, .challengeContribute and .importResponse on the device through the real addon
// (tests/test_node_ptau_challenge.py). Per curve, in ONE process, the round trip from the committed power-5 c1 file runs unpatched and under
// registerAll(snarkjs, { ptauChallenge: true }), both under the same pinned getRandomValues stream:
//   1  registerAll(snarkjs) leaves the three functions the reference's; { ptauChallenge: true } replaces them
//   2  every step: the same bytes and returned value, the committed golden file, to a { type: "mem" } descriptor and from a path to a path
//   3  the imported file passes the reference's powersOfTau.verify; unregister restores the reference's functions
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/ptau_challenge_gpu.js
"use strict";
const fs = require("fs"), os = require("os"), path = require("path");
const L = require("./ptau_verify_lib.js");
process.env.NTHREADS = process.env.NTHREADS || "8";
const snarkjs = require(path.join(L.ROOT, "oracle", "ref_shim.js"));
const { registerAll, unregister } = require(path.join(L.ROOT, "snarkjs_amd", "js", "register.js"));
const GOLD = JSON.parse(fs.readFileSync(path.join(L.ROOT, "tests", "golden", "ptau_challenge_golden.json")));
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }
const same = (a, b) => a.byteLength === b.byteLength && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;
const bytes = (m) => { const d = m.data; return (d instanceof Uint8Array) ? d : d.slice(0, d.byteLength); };
const hex = (b) => (b === undefined || b === null ? String(b) : Buffer.from(b).toString("hex"));
const KEYS = ["exportChallenge", "challengeContribute", "importResponse"];
const NAMES = ["old.ptau", "challenge", "response", "new.ptau", "bare.ptau"];
L.subtleShim();

// the round trip through whatever is installed: [{ ret, data }] for the challenge, the response and the two imports; with a directory, from path to path
async function trip(curve, old, g, dir) {
    snarkjs.reseed();
    const at = (i) => (dir ? path.join(dir, NAMES[i]) : { type: "mem" });
    const read = (t) => (dir ? new Uint8Array(fs.readFileSync(t)) : bytes(t));
    const src = (t) => (dir ? t : { type: "mem", data: bytes(t) });
    const t = [at(0), at(1), at(2), at(3), at(4)], out = [], P = snarkjs.powersOfTau;
    if (dir) fs.writeFileSync(t[0], old); else t[0].data = new Uint8Array(old);
    out.push({ ret: await P.exportChallenge(src(t[0]), t[1]), data: read(t[1]) });
    out.push({ ret: await P.challengeContribute(curve, src(t[1]), t[2], g.entropy), data: read(t[2]) });
    out.push({ ret: await P.importResponse(src(t[0]), src(t[2]), t[3], g.name, true), data: read(t[3]) });
    out.push({ ret: await P.importResponse(src(t[0]), src(t[2]), t[4], g.name, false), data: read(t[4]) });
    return out;
}

async function main() {
    const orig = {};
    for (const k of KEYS) orig[k] = snarkjs.powersOfTau[k];
    const tmp = fs.mkdtempSync(path.join(os.tmpdir(), "ptau_challenge_"));
    try {
        for (const name of ["bn128", "bls12381"]) {
            const curve = await snarkjs.curves.getCurveFromName(name), g = GOLD.trips[`${name}_p5`], old = L.G(g.from);
            const ref = await trip(curve, old, g, null);
            await registerAll(snarkjs);
            check(`${name}: registerAll(snarkjs) keeps the reference's functions`, KEYS.every((k) => snarkjs.powersOfTau[k] === orig[k]));
            await registerAll(snarkjs, { ptauChallenge: true });
            check(`${name}: { ptauChallenge: true } replaces them`, KEYS.every((k) => snarkjs.powersOfTau[k] !== orig[k]));
            const dev = await trip(curve, old, g, null), viaPath = await trip(curve, old, g, tmp);
            const labels = ["exportChallenge", "challengeContribute", "importResponse", "importResponse without points"], files = ["challenge", "response", "imported", "nopoints"];
            for (let i = 0; i < 4; i++) {
                check(`${name}: ${labels[i]}: the reference's bytes and returned value`, same(dev[i].data, ref[i].data) && hex(dev[i].ret) === hex(ref[i].ret));
                check(`${name}: ${labels[i]}: from a path to a path`, same(viaPath[i].data, ref[i].data) && hex(viaPath[i].ret) === hex(ref[i].ret));
                check(`${name}: ${labels[i]}: the committed golden file`, same(dev[i].data, L.G(g.files[files[i]].file)));
            }
            check(`${name}: the recorded hashes`, hex(dev[0].ret) === g.challengeHash && hex(dev[2].ret) === g.nextChallenge && hex(dev[3].ret) === g.noPointsReturned);
            let msg = "";
            try { await snarkjs.powersOfTau.exportChallenge(path.join(tmp, NAMES[4]), { type: "mem" }); } catch (e) { msg = e.message; }
            check(`${name}: export from the file without points fails with the file's name in front`, msg === `${path.join(tmp, NAMES[4])}: Missing section 2`, msg);
            unregister(snarkjs);
            for (const c of ["bn128", "bls12381"]) unregister(await snarkjs.curves.getCurveFromName(c));      // registerAll patched both curve objects
            check(`${name}: unregister restores the reference's functions`, KEYS.every((k) => snarkjs.powersOfTau[k] === orig[k]));
            check(`${name}: the reference's verify accepts the file imported on the device`, (await snarkjs.powersOfTau.verify({ type: "mem", data: dev[2].data })) === true);
        }
    } finally {
        for (const n of NAMES) if (fs.existsSync(path.join(tmp, n))) fs.unlinkSync(path.join(tmp, n));
        fs.rmdirSync(tmp);
    }
    console.log(fails ? `${fails} FAILED` : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.error(e); process.exit(1); });
