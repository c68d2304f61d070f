// tests/js/aggregate_verify_gpu.js — the aggregated PLONK / FFLONK check from Node on the GPU box: VerifyingKey.verifyAll against
// VerifyingKey.verifyMany of the same key. argv[2]: a JSON file written by tests/test_node_aggregate_verify.py:
// [{protocol, vk, golden: {publicSignals, proof}, cases: [{label, publicSignals, proof}]}].
//   1  verifyAll of the golden proof alone and eight times over is true; of no proof at all is true
//   2  for every tamper t: verifyAll([golden, t, golden]) === verifyMany([golden, t, golden]).every(Boolean), under a fixed and under an OS seed
//   3  a seed of another length is refused
// Run:  node tests/js/aggregate_verify_gpu.js cases.json
"use strict";
const fs = require("fs"), path = require("path");
const ROOT = path.join(__dirname, "..", "..");
const KEYS = { plonk: require(path.join(ROOT, "snarkjs_amd", "js", "plonk_verify_native.js")).VerifyingKey,
               fflonk: require(path.join(ROOT, "snarkjs_amd", "js", "fflonk_verify_native.js")).VerifyingKey };
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }

async function main() {
    const sets = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
    const seed = Uint8Array.from({ length: 32 }, (_, i) => 7 * i + 1);
    for (const s of sets) {
        const key = new KEYS[s.protocol](s.vk, { device: 0 });
        const g = s.golden;
        check(s.name + " golden alone", (await key.verifyAll([g.publicSignals], [g.proof], { seed })) === true);
        check(s.name + " golden x 8", (await key.verifyAll(new Array(8).fill(g.publicSignals), new Array(8).fill(g.proof))) === true);
        check(s.name + " empty", (await key.verifyAll([], [])) === true);
        let seen = { t: 0, f: 0 };
        for (const c of s.cases) {
            let want, got, got2;
            if (c.publicSignals.length !== g.publicSignals.length) {                 // a batch carries one signal count: the tamper alone
                want = (await key.verifyMany([c.publicSignals], [c.proof])).every(Boolean);
                got = await key.verifyAll([c.publicSignals], [c.proof], { seed });
                got2 = got;
            } else {
                const sigs = [g.publicSignals, c.publicSignals, g.publicSignals], proofs = [g.proof, c.proof, g.proof];
                want = (await key.verifyMany(sigs, proofs)).every(Boolean);
                got = await key.verifyAll(sigs, proofs, { seed });
                got2 = await key.verifyAll(sigs, proofs);
            }
            seen[want ? "t" : "f"]++;
            check(s.name + " " + c.label, got === want && got2 === want, JSON.stringify({ want, got, got2 }));
        }
        check(s.name + " both outcomes seen", seen.t > 0 && seen.f > 0, JSON.stringify(seen));
        let refused = false;
        try { await key.verifyAll([g.publicSignals], [g.proof], { seed: new Uint8Array(5) }); } catch (e) { refused = /32 bytes/.test(e.message); }
        check(s.name + " short seed refused", refused);
        key.release();
    }
    console.log(fails ? "FAILED " + fails : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.log("FAIL", e && e.stack || e); process.exit(1); });
