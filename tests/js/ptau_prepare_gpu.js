// tests/js/ptau_prepare_gpu.js — snarkjs.powersOfTau.preparePhase2 and .convert on the device through the real addon (tests/test_node_ptau_prepare.py). Per
// curve, in ONE process, both functions run unpatched and under registerAll(snarkjs, { ptauPrepare: true }) on the p6 and p8 files:
//   1  registerAll(snarkjs) leaves the two functions the reference's; { ptauPrepare: true } replaces them
//   2  preparePhase2 of the raw p6 ceremony and of the p8 setup file, convert of the prepared p6 file without its top block and of the p8 file: the same bytes,
//      to a { type: "mem" } descriptor and to a path
//   3  unregister restores the reference's functions
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/ptau_prepare_gpu.js
"use strict";
const fs = require("fs"), os = require("os"), path = require("path");
const L = require("./ptau_verify_lib.js");
process.env.NTHREADS = process.env.NTHREADS || "8";
const snarkjs = require(path.join(L.ROOT, "oracle", "ref_shim.js"));
const { registerAll, unregister } = require(path.join(L.ROOT, "snarkjs_amd", "js", "register.js"));
const setupN = require(path.join(L.ROOT, "snarkjs_amd", "js", "groth16_setup_native.js"));
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }
const same = (a, b) => a.byteLength === b.byteLength && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;
const bytes = (m) => { const d = m.data; return (d instanceof Uint8Array) ? d : d.slice(0, d.byteLength); };

function casesOf(name, cv) {
    const p6raw = L.G(`ptau_${name}_p6_c3b_raw.ptau`), p6 = L.G(`ptau_${name}_p6_c3b.ptau`), p8 = L.G(`setup_${name}_p8.ptau`);
    const noTop = L.join(p6, L.split(p6).map(([t, b]) => [t, t == 12 ? b.subarray(0, b.length - 128 * 2 * cv.n8q) : b]));
    return [["preparePhase2", "raw p6", p6raw, p6], ["preparePhase2", "p8", p8, p8], ["convert", "p6 without its top block", noTop, p6], ["convert", "p8", p8, null]];
}
async function runAll(name, cv) {
    const out = {};
    for (const [which, label, raw] of casesOf(name, cv)) {
        const mem = { type: "mem" };
        const ret = await snarkjs.powersOfTau[which]({ type: "mem", data: raw }, mem);
        out[`${which}(${label})`] = { ret, data: bytes(mem) };
    }
    return out;
}

async function main() {
    const orig = { preparePhase2: snarkjs.powersOfTau.preparePhase2, convert: snarkjs.powersOfTau.convert };
    const tmp = fs.mkdtempSync(path.join(os.tmpdir(), "ptau_prepare_"));
    try {
        for (const name of ["bn128", "bls12381"]) {
            const cv = setupN.CURVES.find((c) => c.name === name);
            await snarkjs.curves.getCurveFromName(name);
            const ref = await runAll(name, cv);
            await registerAll(snarkjs);
            check(`${name}: registerAll(snarkjs) keeps the reference's functions`, snarkjs.powersOfTau.preparePhase2 === orig.preparePhase2 && snarkjs.powersOfTau.convert === orig.convert);
            await registerAll(snarkjs, { ptauPrepare: true });
            check(`${name}: { ptauPrepare: true } replaces them`, snarkjs.powersOfTau.preparePhase2 !== orig.preparePhase2 && snarkjs.powersOfTau.convert !== orig.convert);
            const dev = await runAll(name, cv);
            for (const [which, label, raw, want] of casesOf(name, cv)) {
                const k = `${which}(${label})`;
                check(`${name}: ${k}: the reference's bytes`, same(dev[k].data, ref[k].data) && dev[k].ret === ref[k].ret);
                if (want) check(`${name}: ${k}: the committed file`, same(dev[k].data, want));
                else check(`${name}: ${k}: not the file itself`, !same(dev[k].data, raw) && dev[k].data.byteLength === raw.byteLength + 512 * 2 * cv.n8q);
                const src = path.join(tmp, "old.ptau"), dst = path.join(tmp, "new.ptau");
                fs.writeFileSync(src, raw);
                await snarkjs.powersOfTau[which](src, dst);
                check(`${name}: ${k}: from a path to a path`, same(new Uint8Array(fs.readFileSync(dst)), ref[k].data));
            }
            unregister(snarkjs);
            for (const c of ["bn128", "bls12381"]) unregister(await snarkjs.curves.getCurveFromName(c));      // registerAll patched both curve objects
            check(`${name}: unregister restores the reference's functions`, snarkjs.powersOfTau.preparePhase2 === orig.preparePhase2 && snarkjs.powersOfTau.convert === orig.convert);
        }
    } finally {
        for (const f of ["old.ptau", "new.ptau"]) if (fs.existsSync(path.join(tmp, f))) fs.unlinkSync(path.join(tmp, f));
        fs.rmdirSync(tmp);
    }
    console.log(fails ? `${fails} FAILED` : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.error(e); process.exit(1); });
