// tests/js/bellman_gpu.js — snarkjs.zKey.exportBellman, .bellmanContribute and .importBellman on the device through the real addon (tests/test_node_bellman.py).
// Per curve and circuit, in ONE process, the round trip from the committed c1 key runs unpatched and under registerAll(snarkjs, { bellman: true }), both under
// the same pinned getRandomValues stream:
//   1  registerAll(snarkjs) leaves the three functions the reference's; { bellman: true } replaces them, also beside { setup, phase2, phase2Verify }
//   2  every step: the same bytes, returned value and logger lines, to a { type: "mem" } descriptor and from a path to a path; the committed challenge
//   3  with the recorded draw the driver writes the golden response and the recorded key; the reference's verifyFromInit accepts the key imported on the device
//   4  unregister restores the reference's functions
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/bellman_gpu.js
"use strict";
const fs = require("fs"), os = require("os"), path = require("path"), crypto = require("crypto");
const L = require("./ptau_verify_lib.js");
process.env.NTHREADS = process.env.NTHREADS || "8";
const snarkjs = require(path.join(L.ROOT, "oracle", "ref_shim.js"));
const { registerAll, unregister } = require(path.join(L.ROOT, "snarkjs_amd", "js", "register.js"));
const bN = require(path.join(L.ROOT, "snarkjs_amd", "js", "groth16_bellman_native.js"));
const GOLD = JSON.parse(fs.readFileSync(path.join(L.ROOT, "tests", "golden", "bellman_golden.json")));
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }
const same = (a, b) => a.byteLength === b.byteLength && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;
const bytes = (m) => { const d = m.data; return (d instanceof Uint8Array) ? d : d.slice(0, d.byteLength); };
const hex = (b) => (b === undefined || b === null || typeof b === "boolean" ? String(b) : Buffer.from(b).toString("hex"));
const sha = (b) => crypto.createHash("sha256").update(b).digest("hex");
const KEYS = ["exportBellman", "bellmanContribute", "importBellman"];
const NAMES = ["old.zkey", "challenge.params", "response.params", "new.zkey"];

// the round trip through whatever is installed: [{ ret, data, lines }] for the challenge, the response and the key; with a directory, from path to path
async function trip(curve, key, entropy, name, dir) {
    snarkjs.reseed();
    const at = (i) => (dir ? path.join(dir, NAMES[i]) : { type: "mem" });
    const read = (t) => (dir ? new Uint8Array(fs.readFileSync(t)) : bytes(t));
    const src = (t) => (dir ? t : { type: "mem", data: bytes(t) });
    const t = [at(0), at(1), at(2), at(3)], out = [], Z = snarkjs.zKey;
    if (dir) fs.writeFileSync(t[0], key); else t[0].data = new Uint8Array(key);
    const logged = () => { const lines = [], push = (level) => (text) => lines.push([level, text]); return { lines, logger: { debug: () => {}, info: push("info"), warn: push("warn"), error: push("error") } }; };
    let lg = logged();
    out.push({ ret: await Z.exportBellman(src(t[0]), t[1], lg.logger), data: read(t[1]), lines: lg.lines });
    lg = logged();
    out.push({ ret: await Z.bellmanContribute(curve, src(t[1]), t[2], entropy, lg.logger), data: read(t[2]), lines: lg.lines });
    lg = logged();
    out.push({ ret: await Z.importBellman(src(t[0]), src(t[2]), t[3], name, lg.logger), data: read(t[3]), lines: lg.lines });
    return out;
}

async function main() {
    const orig = {};
    for (const k of KEYS) orig[k] = snarkjs.zKey[k];
    const tmp = fs.mkdtempSync(path.join(os.tmpdir(), "bellman_"));
    try {
        for (const name of ["bn128", "bls12381"]) {
            const curve = await snarkjs.curves.getCurveFromName(name);
            for (const circuit of ["full", "edge"]) {
                const key = L.G(`phase2_${name}_${circuit}_c1.zkey`), g = GOLD.files[`bellman_${name}_${circuit}_response.params`], imp = GOLD.imported[`${name}_${circuit}`];
                const ref = await trip(curve, key, g.entropy, imp.name, null);
                await registerAll(snarkjs);
                check(`${name} ${circuit}: registerAll(snarkjs) keeps the reference's functions`, KEYS.every((k) => snarkjs.zKey[k] === orig[k]));
                await registerAll(snarkjs, circuit == "full" ? { bellman: true } : { bellman: true, setup: true, phase2: true, phase2Verify: true });
                check(`${name} ${circuit}: { bellman: true } replaces them`, KEYS.every((k) => snarkjs.zKey[k] !== orig[k]));
                const dev = await trip(curve, key, g.entropy, imp.name, null), viaPath = await trip(curve, key, g.entropy, imp.name, tmp);
                const labels = ["exportBellman", "bellmanContribute", "importBellman"];
                for (let i = 0; i < 3; i++) {
                    check(`${name} ${circuit}: ${labels[i]}: the reference's bytes, returned value and lines`, same(dev[i].data, ref[i].data) && hex(dev[i].ret) === hex(ref[i].ret) && L.sameLines(dev[i].lines, ref[i].lines));
                    check(`${name} ${circuit}: ${labels[i]}: from a path to a path`, same(viaPath[i].data, ref[i].data) && hex(viaPath[i].ret) === hex(ref[i].ret));
                }
                check(`${name} ${circuit}: the committed challenge`, same(dev[0].data, L.G(`bellman_${name}_${circuit}_challenge.params`)) && dev[2].ret === true);
                const direct = await bN.bellmanContribute(curve, L.G(g.from), g.entropy, { random64: Buffer.from(g.random64, "hex") });
                const key2 = await bN.importBellman(key, direct.response, imp.name, {});
                check(`${name} ${circuit}: with the recorded draw: the golden response, hash and key`, same(direct.response, L.G(`bellman_${name}_${circuit}_response.params`)) && hex(direct.contributionHash) === g.contributionHash && sha(key2.zkey) === imp.sha256);
                unregister(snarkjs);
                for (const c of ["bn128", "bls12381"]) unregister(await snarkjs.curves.getCurveFromName(c));      // registerAll patched both curve objects
                check(`${name} ${circuit}: unregister restores the reference's functions`, KEYS.every((k) => snarkjs.zKey[k] === orig[k]) && !snarkjs.__zkmiBellman);
                const verdict = await snarkjs.zKey.verifyFromInit({ type: "mem", data: L.G(`setup_${name}_${circuit}.zkey`) }, { type: "mem", data: L.G(`setup_${name}_p8.ptau`) }, { type: "mem", data: dev[2].data });
                check(`${name} ${circuit}: the reference's verifyFromInit accepts the key imported on the device`, verdict === true);
            }
        }
    } finally {
        for (const n of NAMES) if (fs.existsSync(path.join(tmp, n))) fs.unlinkSync(path.join(tmp, n));
        fs.rmdirSync(tmp);
    }
    console.log(fails ? `${fails} FAILED` : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.error(e); process.exit(1); });
