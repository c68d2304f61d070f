// tools/phase2verifybench_ref.js — the reference leg of tools/phase2verifybench.py: the reference's own WASM zKey.verifyFromInit on the three given files, on
// this box's host cores.
//   node --harmony-optional-chaining --harmony-nullish tools/phase2verifybench_ref.js init.zkey pot.ptau key.zkey reps
//   ->  one JSON line {ms: [per run, after one warm-up], threads, verdicts}
'use strict';
const fs = require('fs'), path = require('path');
const snarkjs = require(path.join(__dirname, '..', 'oracle', 'ref_shim.js'));
(async () => {
    const [init, ptau, key] = [2, 3, 4].map((i) => new Uint8Array(fs.readFileSync(process.argv[i])));
    const reps = parseInt(process.argv[5] || '5');
    await snarkjs.curves.getCurveFromName('bn128');                  // worker start-up outside the timed part
    const ms = [], verdicts = [];
    for (let i = 0; i <= reps; i++) {
        const t0 = process.hrtime.bigint();
        const ok = await snarkjs.zKey.verifyFromInit(init, ptau, key);
        if (i) { ms.push(Number(process.hrtime.bigint() - t0) / 1e6); verdicts.push(ok); }
    }
    console.log(JSON.stringify({ ms, threads: snarkjs.nThreads, verdicts }));
    process.exit(0);
})().catch(e => { console.error(e); process.exit(1); });
