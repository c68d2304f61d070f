// tools/ptaupreparebench_ref.js — the reference legs of tools/ptaupreparebench.py, on this box's host cores:
//   node --harmony-optional-chaining --harmony-nullish tools/ptaupreparebench_ref.js make <power> <out.ptau>
//       unmodified snarkjs (with the drop-in for its bulk curve methods, not timed as part of any leg): newAccumulator -> contribute on BN254, the RAW file
//       written to <out.ptau>; one JSON line {bytes, seconds, made_by}
//   node --harmony-optional-chaining --harmony-nullish tools/ptaupreparebench_ref.js prepare <file.ptau> <reps> <plain | dropin> <cap seconds>
//       powersOfTau.preparePhase2 of unmodified snarkjs, on plain WASM or with registerAll(snarkjs) alone; one JSON line
//       {ms: [per run after one warm-up], threads, sha256, capped}. A warm-up that takes longer than the cap is reported as the one run (capped: true).
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const snarkjs = require(path.join(__dirname, '..', 'oracle', 'ref_shim.js'));
const bytes = (m) => { const d = m.data; return (d instanceof Uint8Array) ? d : d.slice(0, d.byteLength); };
(async () => {
    const curve = await snarkjs.curves.getCurveFromName('bn128');     // worker start-up outside the timed part
    const register = () => require(path.join(__dirname, '..', 'snarkjs_amd', 'js', 'register.js')).registerAll(snarkjs);
    if (process.argv[2] === 'make') {
        let madeBy = 'unmodified snarkjs with the drop-in';
        try { await register(); } catch (e) { madeBy = 'the reference alone (drop-in not loaded: ' + e.message + ')'; }
        const t0 = process.hrtime.bigint(), a = { type: 'mem' }, b = { type: 'mem' };
        await snarkjs.powersOfTau.newAccumulator(curve, parseInt(process.argv[3]), a);
        await snarkjs.powersOfTau.contribute(a, b, 'bench', 'Entropy');
        const raw = bytes(b);
        fs.writeFileSync(process.argv[4], raw);
        console.log(JSON.stringify({ bytes: raw.length, seconds: Number(process.hrtime.bigint() - t0) / 1e9, made_by: madeBy }));
    } else {
        const raw = new Uint8Array(fs.readFileSync(process.argv[3])), reps = parseInt(process.argv[4] || '5'), cap = parseFloat(process.argv[6] || '60');
        if (process.argv[5] === 'dropin') await register();
        const ms = [];
        let sha = null, capped = false;
        for (let i = 0; i <= reps; i++) {
            const out = { type: 'mem' }, t0 = process.hrtime.bigint();
            await snarkjs.powersOfTau.preparePhase2({ type: 'mem', data: raw }, out);
            const t = Number(process.hrtime.bigint() - t0) / 1e6, h = crypto.createHash('sha256').update(bytes(out)).digest('hex');
            if (sha !== null && h !== sha) throw new Error('two runs gave different bytes');
            sha = h;
            if (i) ms.push(t);
            else if (t > cap * 1e3) { ms.push(t); capped = true; break; }
        }
        console.log(JSON.stringify({ ms, threads: snarkjs.nThreads, sha256: sha, capped }));
    }
    process.exit(0);
})().catch(e => { console.error(e); process.exit(1); });
