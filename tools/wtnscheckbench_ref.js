// tools/wtnscheckbench_ref.js — the reference leg of tools/wtnscheckbench.py, on this box's host cores:
//   node --harmony-optional-chaining --harmony-nullish tools/wtnscheckbench_ref.js <r1cs file> <wtns file> <reps> <cap seconds>
//       wtns.check(r1cs, wtns) of unmodified snarkjs on the two files (read outside the timed part, no logger); one JSON line
//       {ms: [per run after one warm-up], verdict, capped}. A warm-up that takes longer than the cap is reported as the one run (capped: true).
'use strict';
const path = require('path'), fs = require('fs');
const snarkjs = require(path.join(__dirname, '..', 'oracle', 'ref_shim.js'));
(async () => {
    const reps = parseInt(process.argv[4] || '5'), cap = parseFloat(process.argv[5] || '120');
    await snarkjs.curves.getCurveFromName('bn128');                   // curve start-up outside the timed part
    const r1cs = new Uint8Array(fs.readFileSync(process.argv[2])), wtns = new Uint8Array(fs.readFileSync(process.argv[3])), ms = [];
    const quiet = { debug() {}, info() {}, warn() {}, error() {} };   // a bad witness needs a logger to come back at all
    let verdict = null, capped = false;
    for (let i = 0; i <= reps; i++) {
        const t0 = process.hrtime.bigint();
        const v = await snarkjs.wtns.check(r1cs, wtns, quiet);
        const t = Number(process.hrtime.bigint() - t0) / 1e6;
        if (verdict !== null && v !== verdict) throw new Error('two runs gave different verdicts');
        verdict = v;
        if (i) ms.push(t);
        else if (t > cap * 1e3) { ms.push(t); capped = true; break; }
    }
    console.log(JSON.stringify({ ms, verdict, capped }));
    process.exit(0);
})().catch(e => { console.error(e); process.exit(1); });
