// tools/ptauverifybench_ref.js — the reference legs of tools/ptauverifybench.py, on this box's host cores:
//   node --harmony-optional-chaining --harmony-nullish tools/ptauverifybench_ref.js make <power> <out.ptau>
//       unmodified snarkjs with the drop-in (registerAll(snarkjs): its bulk curve methods on the device): newAccumulator -> contribute -> preparePhase2 on
//       BN254, written to <out.ptau>; one JSON line {bytes, seconds, made_by}. If the drop-in cannot be loaded the reference makes the file alone and says so.
//   node --harmony-optional-chaining --harmony-nullish tools/ptauverifybench_ref.js verify <file.ptau> <reps>
//       the reference's WASM powersOfTau.verify; one JSON line {ms: [per run, after one warm-up], threads, verdicts}
'use strict';
const fs = require('fs'), path = require('path');
const snarkjs = require(path.join(__dirname, '..', 'oracle', 'ref_shim.js'));
(async () => {
    const curve = await snarkjs.curves.getCurveFromName('bn128');     // worker start-up outside the timed part
    if (process.argv[2] === 'make') {
        let madeBy = 'unmodified snarkjs with the drop-in';
        try { await require(path.join(__dirname, '..', 'snarkjs_amd', 'js', 'register.js')).registerAll(snarkjs); } catch (e) { madeBy = 'the reference alone (drop-in not loaded: ' + e.message + ')'; }
        const t0 = process.hrtime.bigint(), a = { type: 'mem' }, b = { type: 'mem' }, c = { type: 'mem' };
        await snarkjs.powersOfTau.newAccumulator(curve, parseInt(process.argv[3]), a);
        await snarkjs.powersOfTau.contribute(a, b, 'bench', 'Entropy');
        await snarkjs.powersOfTau.preparePhase2(b, c);
        fs.writeFileSync(process.argv[4], c.data);
        console.log(JSON.stringify({ bytes: c.data.length, seconds: Number(process.hrtime.bigint() - t0) / 1e9, made_by: madeBy }));
    } else {
        const raw = new Uint8Array(fs.readFileSync(process.argv[3])), reps = parseInt(process.argv[4] || '5');
        const ms = [], verdicts = [];
        for (let i = 0; i <= reps; i++) {
            const t0 = process.hrtime.bigint();
            const ok = await snarkjs.powersOfTau.verify({ type: 'mem', data: raw });
            if (i) { ms.push(Number(process.hrtime.bigint() - t0) / 1e6); verdicts.push(ok); }
        }
        console.log(JSON.stringify({ ms, threads: snarkjs.nThreads, verdicts }));
    }
    process.exit(0);
})().catch(e => { console.error(e); process.exit(1); });
