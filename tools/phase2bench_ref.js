// tools/phase2bench_ref.js — the reference leg of tools/phase2bench.py: the reference's own WASM zKey.contribute on the given key, on this box's host cores.
//   node --harmony-optional-chaining --harmony-nullish tools/phase2bench_ref.js key.zkey name entropy  ->  one JSON line {ms, threads, sha256, contributionHash, random64}
// random64: the 64 bytes contribute drew from getRandomValues, so that the device leg can repeat the call.
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const snarkjs = require(path.join(__dirname, '..', 'oracle', 'ref_shim.js'));
(async () => {
    const old = { type: 'mem', data: new Uint8Array(fs.readFileSync(process.argv[2])) }, z = { type: 'mem' };
    let random64 = null;
    const plain = globalThis.crypto.getRandomValues;
    globalThis.crypto.getRandomValues = a => { const r = plain(a); if (a.byteLength === 64) random64 = Buffer.from(a.buffer, a.byteOffset, 64).toString('hex'); return r; };
    await snarkjs.curves.getCurveFromName('bn128');                  // worker start-up outside the timed part (the curve of the key is built on demand)
    const t0 = process.hrtime.bigint();
    const h = await snarkjs.zKey.contribute(old, z, process.argv[3], process.argv[4]);
    const ms = Number(process.hrtime.bigint() - t0) / 1e6;
    const data = z.data instanceof Uint8Array ? z.data : z.data.slice(0, z.data.byteLength);
    console.log(JSON.stringify({ ms, threads: snarkjs.nThreads, sha256: crypto.createHash('sha256').update(data).digest('hex'), contributionHash: Buffer.from(h).toString('hex'), random64 }));
    process.exit(0);
})().catch(e => { console.error(e); process.exit(1); });
