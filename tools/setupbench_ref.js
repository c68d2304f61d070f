// tools/setupbench_ref.js — the reference leg of tools/setupbench.py: the reference's own WASM zKey.newZKey (or, with --protocol plonk | fflonk, plonk.setup | fflonk.setup) on the given files, on this box's host cores.
//   node --harmony-optional-chaining --harmony-nullish tools/setupbench_ref.js circuit.r1cs prepared.ptau [--protocol plonk|fflonk]  ->  one JSON line {ms, sha256, csHash}
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const snarkjs = require(path.join(__dirname, '..', 'oracle', 'ref_shim.js'));
(async () => {
    const z = { type: 'mem' };
    // the bundle is the browser build, which reads a string as a URL: load both files first, outside the timed part
    const r1cs = new Uint8Array(fs.readFileSync(process.argv[2])), ptau = new Uint8Array(fs.readFileSync(process.argv[3]));
    const t0 = process.hrtime.bigint();
    const protocol = process.argv[4] === '--protocol' ? process.argv[5] : 'groth16', plonk = protocol !== 'groth16';
    const h = protocol === 'fflonk' ? await snarkjs.fflonk.setup(r1cs, ptau, z) : plonk ? await snarkjs.plonk.setup(r1cs, ptau, z) : await snarkjs.zKey.newZKey(r1cs, ptau, z);
    const ms = Number(process.hrtime.bigint() - t0) / 1e6;
    if (h === -1) throw new Error('the reference refused the inputs');
    const data = z.data instanceof Uint8Array ? z.data : z.data.slice(0, z.data.byteLength);
    console.log(JSON.stringify({ ms, threads: snarkjs.nThreads, sha256: crypto.createHash('sha256').update(data).digest('hex'), csHash: plonk ? null : Buffer.from(h).toString('hex') }));
    process.exit(0);
})().catch(e => { console.error(e); process.exit(1); });
