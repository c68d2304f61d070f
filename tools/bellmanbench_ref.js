// tools/bellmanbench_ref.js — the reference leg of tools/bellmanbench.py: the reference's own WASM zKey.exportBellman, bellmanContribute and importBellman on the
// given key, on this box's host cores.
//   node --harmony-optional-chaining --harmony-nullish tools/bellmanbench_ref.js key.zkey curve entropy name
//   ->  one JSON line {ms: [export, contribute, import], threads, sha256: [challenge, response, key], contributionHash, random64}
// random64: the 64 bytes bellmanContribute drew from getRandomValues, so that the device leg can repeat the call.
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const snarkjs = require(path.join(__dirname, '..', 'oracle', 'ref_shim.js'));
(async () => {
    const key = new Uint8Array(fs.readFileSync(process.argv[2])), mem = d => ({ type: 'mem', data: d });
    const flat = f => (f.data instanceof Uint8Array ? f.data : f.data.slice(0, f.data.byteLength));
    const sha = b => crypto.createHash('sha256').update(b).digest('hex');
    let random64 = null;
    const plain = globalThis.crypto.getRandomValues;
    globalThis.crypto.getRandomValues = a => { const r = plain(a); if (a.byteLength === 64) random64 = Buffer.from(a.buffer, a.byteOffset, 64).toString('hex'); return r; };
    const curve = await snarkjs.curves.getCurveFromName(process.argv[3]);     // worker start-up outside the timed part
    const ms = [], timed = async f => { const t0 = process.hrtime.bigint(); const r = await f(); ms.push(Number(process.hrtime.bigint() - t0) / 1e6); return r; };
    const ch = { type: 'mem' }, rs = { type: 'mem' }, nw = { type: 'mem' };
    await timed(() => snarkjs.zKey.exportBellman(mem(key), ch));
    const h = await timed(() => snarkjs.zKey.bellmanContribute(curve, mem(flat(ch)), rs, process.argv[4]));
    const ok = await timed(() => snarkjs.zKey.importBellman(mem(key), mem(flat(rs)), nw, process.argv[5]));
    if (ok !== true) throw new Error('importBellman refused the response');
    console.log(JSON.stringify({ ms, threads: snarkjs.nThreads, sha256: [sha(flat(ch)), sha(flat(rs)), sha(flat(nw))], contributionHash: Buffer.from(h).toString('hex'), random64 }));
    process.exit(0);
})().catch(e => { console.error(e); process.exit(1); });
