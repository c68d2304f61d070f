// tools/ref_wasm_verify.js — the reference's own groth16.verify (WASM, the bundle staged in oracle/_ref/) timed on this host, one proof at a
// time on one thread: the baseline of tools/verifybench.py, measured in the same run. Prints one JSON line {curve: {per_s, ms_per_proof, n}}.
// A second argument "plonk" or "fflonk" times plonk.verify / fflonk.verify on their goldens instead.
// Run:  SINGLE=1 node --harmony-optional-chaining --harmony-nullish tools/ref_wasm_verify.js [count] [plonk|fflonk]
"use strict";
const path = require("path");
const ROOT = path.join(__dirname, "..");
process.env.SINGLE = "1";
const snarkjs = require(path.join(ROOT, "oracle", "ref_shim.js"));
async function main() {
    const count = Number(process.argv[2] || 20), out = {};
    const proto = ["plonk", "fflonk"].includes(process.argv[3]) ? process.argv[3] : "groth16", mod = snarkjs[proto];
    const files = { groth16: ["groth16_bn128_n1024.json", "groth16_bls12381_n1024.json"], plonk: ["plonk_bn128_n2048.json", "plonk_bls12381_small.json"],
                    fflonk: ["fflonk_bn128_n256.json"] };
    for (const f of files[proto]) {
        const d = require(path.join(ROOT, "tests", "golden", f));
        for (let i = 0; i < 3; i++) if (!(await mod.verify(d.vk, d.publicSignals, d.proof))) throw new Error("golden proof rejected");   // warm-up
        const t = process.hrtime.bigint();
        for (let i = 0; i < count; i++) await mod.verify(d.vk, d.publicSignals, d.proof);
        const s = Number(process.hrtime.bigint() - t) / 1e9;
        out[d.vk.curve] = { per_s: +(count / s).toFixed(2), ms_per_proof: +(1000 * s / count).toFixed(2), n: count };
    }
    console.log(JSON.stringify(out));
    process.exit(0);
}
main().catch((e) => { console.error(e); process.exit(1); });
