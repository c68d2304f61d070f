// tests/js/groth16_aggregate_verify_gpu.js — the aggregated Groth16 check from Node on the GPU box: VerifyingKey.verifyAll against
// VerifyingKey.verifyMany of the same key. argv[2]: a JSON file written by tests/test_node_groth16_aggregate.py:
// [{name, vk, publicSignals, proofs: [130 valid], tampered}].
//   1  for n in 1, 65, 130: verifyAll(first n) === verifyMany(first n).every(Boolean) === true, under a fixed and under an OS seed
//   2  the same with the tampered proof at a position of the batch: both false, and verifyMany names that position only
//   3  no proof at all is true; a seed of another length and more signals than nPublic are refused
// Run:  node tests/js/groth16_aggregate_verify_gpu.js cases.json
"use strict";
const fs = require("fs"), path = require("path");
const ROOT = path.join(__dirname, "..", "..");
const { VerifyingKey } = require(path.join(ROOT, "snarkjs_amd", "js", "groth16_verify_native.js"));
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }

async function main() {
    const sets = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
    const seed = Uint8Array.from({ length: 32 }, (_, i) => 7 * i + 1);
    for (const s of sets) {
        const key = new VerifyingKey(s.vk, { device: 0 });
        for (const n of [1, 65, 130]) {
            const sigs = new Array(n).fill(s.publicSignals), proofs = s.proofs.slice(0, n);
            const many = await key.verifyMany(sigs, proofs);
            check(s.name + " valid x " + n, many.every(Boolean) && (await key.verifyAll(sigs, proofs, { seed })) === true && (await key.verifyAll(sigs, proofs)) === true);
            const at = (n * 5) % 7 % n, bad = proofs.slice();
            bad[at] = s.tampered;
            const many2 = await key.verifyMany(sigs, bad);
            check(s.name + " tampered at " + at + " of " + n, many2.every((v, i) => v === (i !== at)) && (await key.verifyAll(sigs, bad, { seed })) === false &&
                  (await key.verifyAll(sigs, bad)) === false);
        }
        check(s.name + " empty", (await key.verifyAll([], [])) === true);
        let refused = false;
        try { await key.verifyAll([s.publicSignals], [s.proofs[0]], { seed: new Uint8Array(5) }); } catch (e) { refused = /32 bytes/.test(e.message); }
        check(s.name + " short seed refused", refused);
        refused = false;
        try { await key.verifyAll([s.publicSignals.concat(["1"])], [s.proofs[0]], { seed }); } catch (e) { refused = /nPublic/.test(e.message); }
        check(s.name + " more signals refused", refused);
        key.release();
    }
    console.log(fails ? "FAILED " + fails : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.log("FAIL", e && e.stack || e); process.exit(1); });
