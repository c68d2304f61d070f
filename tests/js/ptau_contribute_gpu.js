// tests/js/ptau_contribute_gpu.js — snarkjs.powersOfTau.newAccumulator, .contribute and .beacon on the device through the real addon
// (tests/test_node_ptau_contribute.py). Per curve, in ONE process, the power-5 chain new -> C1 -> C2 -> B3 runs unpatched and under
// registerAll(snarkjs, { ptauContribute: true }), both under the same pinned getRandomValues stream:
//   1  registerAll(snarkjs) leaves the three functions the reference's; { ptauContribute: true } replaces them
//   2  every step: the same bytes and returned hash, the committed golden file, to a { type: "mem" } descriptor and from a path to a path
//   3  the result passes the reference's powersOfTau.verify; unregister restores the reference's functions
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/ptau_contribute_gpu.js
"use strict";
const fs = require("fs"), os = require("os"), path = require("path");
const L = require("./ptau_verify_lib.js");
process.env.NTHREADS = process.env.NTHREADS || "8";
const snarkjs = require(path.join(L.ROOT, "oracle", "ref_shim.js"));
const { registerAll, unregister } = require(path.join(L.ROOT, "snarkjs_amd", "js", "register.js"));
const GOLD = JSON.parse(fs.readFileSync(path.join(L.ROOT, "tests", "golden", "ptau_contribute_golden.json")));
const BEACON = Array.from({ length: 31 }, (_, i) => (i + 1).toString(16).padStart(2, "0")).join("");
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }
const same = (a, b) => a.byteLength === b.byteLength && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;
const bytes = (m) => { const d = m.data; return (d instanceof Uint8Array) ? d : d.slice(0, d.byteLength); };
const hex = (b) => Buffer.from(b).toString("hex");
const KEYS = ["newAccumulator", "contribute", "beacon"];
L.subtleShim();

// the chain through whatever is installed: [{ ret, data }] for new, c1, c2, b3; with a directory, from path to path
async function chain(curve, dir) {
    snarkjs.reseed();
    const at = (i) => (dir ? path.join(dir, `s${i}.ptau`) : { type: "mem" });
    const read = (t) => (dir ? new Uint8Array(fs.readFileSync(t)) : bytes(t));
    const src = (t) => (dir ? t : { type: "mem", data: bytes(t) });
    const t = [at(0), at(1), at(2), at(3)], out = [];
    out.push({ ret: await snarkjs.powersOfTau.newAccumulator(curve, 5, t[0]), data: read(t[0]) });
    out.push({ ret: await snarkjs.powersOfTau.contribute(src(t[0]), t[1], "C1", "Entropy1"), data: read(t[1]) });
    out.push({ ret: await snarkjs.powersOfTau.contribute(src(t[1]), t[2], "C2", "Entropy2"), data: read(t[2]) });
    out.push({ ret: await snarkjs.powersOfTau.beacon(src(t[2]), t[3], "B3", BEACON, 10), data: read(t[3]) });
    return out;
}

async function main() {
    const orig = {};
    for (const k of KEYS) orig[k] = snarkjs.powersOfTau[k];
    const tmp = fs.mkdtempSync(path.join(os.tmpdir(), "ptau_contribute_"));
    try {
        for (const name of ["bn128", "bls12381"]) {
            const curve = await snarkjs.curves.getCurveFromName(name);
            const ref = await chain(curve, null);
            await registerAll(snarkjs);
            check(`${name}: registerAll(snarkjs) keeps the reference's functions`, KEYS.every((k) => snarkjs.powersOfTau[k] === orig[k]));
            await registerAll(snarkjs, { ptauContribute: true });
            check(`${name}: { ptauContribute: true } replaces them`, KEYS.every((k) => snarkjs.powersOfTau[k] !== orig[k]));
            const dev = await chain(curve, null), viaPath = await chain(curve, tmp);
            const labels = ["newAccumulator", "contribute(C1)", "contribute(C2)", "beacon(B3)"], tags = [null, "c1", "c2", "b3"];
            for (let i = 0; i < 4; i++) {
                check(`${name}: ${labels[i]}: the reference's bytes and returned hash`, same(dev[i].data, ref[i].data) && hex(dev[i].ret) === hex(ref[i].ret));
                check(`${name}: ${labels[i]}: from a path to a path`, same(viaPath[i].data, ref[i].data) && hex(viaPath[i].ret) === hex(ref[i].ret));
                if (tags[i]) {
                    const file = `ptau_${name}_p5_${tags[i]}.ptau`;
                    check(`${name}: ${labels[i]}: the committed golden file`, same(dev[i].data, L.G(file)) && hex(dev[i].ret) === GOLD.steps[file].returned);
                }
            }
            const refusedBeacon = await snarkjs.powersOfTau.beacon({ type: "mem", data: dev[1].data }, { type: "mem" }, "X", BEACON, 9);
            check(`${name}: a refused beacon returns false`, refusedBeacon === false);
            unregister(snarkjs);
            for (const c of ["bn128", "bls12381"]) unregister(await snarkjs.curves.getCurveFromName(c));      // registerAll patched both curve objects
            check(`${name}: unregister restores the reference's functions`, KEYS.every((k) => snarkjs.powersOfTau[k] === orig[k]));
            check(`${name}: the reference's verify accepts the ceremony made on the device`, (await snarkjs.powersOfTau.verify({ type: "mem", data: dev[3].data })) === true);
        }
    } finally {
        for (let i = 0; i < 4; i++) if (fs.existsSync(path.join(tmp, `s${i}.ptau`))) fs.unlinkSync(path.join(tmp, `s${i}.ptau`));
        fs.rmdirSync(tmp);
    }
    console.log(fails ? `${fails} FAILED` : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.error(e); process.exit(1); });
