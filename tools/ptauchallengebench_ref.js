// tools/ptauchallengebench_ref.js — the reference legs of tools/ptauchallengebench.py, on this box's host cores:
//   node --harmony-optional-chaining --harmony-nullish tools/ptauchallengebench_ref.js <challenge file> <reps> <plain | dropin> <cap seconds> <random64 hex>
//       powersOfTau.challengeContribute(bn128, challenge, response, 'Entropy') of unmodified snarkjs on that challenge file (read outside the timed part), on plain
//       WASM or with registerAll(snarkjs) alone, every 64-byte getRandomValues draw answered with <random64>; one JSON line
//       {ms: [per run after one warm-up], threads, sha256, capped}. A warm-up that takes longer than the cap is reported as the one run (capped: true).
'use strict';
const path = require('path'), crypto = require('crypto'), fs = require('fs');
const snarkjs = require(path.join(__dirname, '..', 'oracle', 'ref_shim.js'));
const bytes = (m) => { const d = m.data; return (d instanceof Uint8Array) ? d : d.slice(0, d.byteLength); };
(async () => {
    const file = process.argv[2], reps = parseInt(process.argv[3] || '5'), mode = process.argv[4] || 'plain', cap = parseFloat(process.argv[5] || '60');
    const random64 = Buffer.from(process.argv[6], 'hex');
    if (random64.length !== 64) throw new Error('random64 must be 64 bytes of hex');
    const plainRandom = globalThis.crypto.getRandomValues;
    globalThis.crypto.getRandomValues = a => { if (a.byteLength !== 64) return plainRandom(a); new Uint8Array(a.buffer, a.byteOffset, 64).set(random64); return a; };
    const curve = await snarkjs.curves.getCurveFromName('bn128');     // worker start-up outside the timed part
    if (mode === 'dropin') await require(path.join(__dirname, '..', 'snarkjs_amd', 'js', 'register.js')).registerAll(snarkjs);
    const raw = new Uint8Array(fs.readFileSync(file)), ms = [];
    let sha = null, capped = false;
    for (let i = 0; i <= reps; i++) {
        const out = { type: 'mem' }, t0 = process.hrtime.bigint();
        await snarkjs.powersOfTau.challengeContribute(curve, { type: 'mem', data: raw }, out, 'Entropy');
        const t = Number(process.hrtime.bigint() - t0) / 1e6, h = crypto.createHash('sha256').update(bytes(out)).digest('hex');
        if (sha !== null && h !== sha) throw new Error('two runs gave different bytes');
        sha = h;
        if (i) ms.push(t);
        else if (t > cap * 1e3) { ms.push(t); capped = true; break; }
    }
    console.log(JSON.stringify({ ms, threads: snarkjs.nThreads, sha256: sha, capped }));
    process.exit(0);
})().catch(e => { console.error(e); process.exit(1); });
