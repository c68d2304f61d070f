// tools/gen_setup_golden.js — golden vectors of the Groth16 setup (snarkjs_amd/groth16_setup.py, js/groth16_setup_native.js), produced by the
// REFERENCE on the CPU: per curve a prepared power-8 ptau from a seeded ceremony (new -> contribute -> preparePhase2) and the reference's own
// zKey.newZKey output for the two r1cs fixtures that tools/gen_setup_r1cs.py writes.
//   python tools/gen_setup_r1cs.py && node --harmony-optional-chaining --harmony-nullish tools/gen_setup_golden.js
// writes tests/golden/setup_<curve>_p8.ptau, setup_<curve>_{edge,full}.zkey and setup_golden.json (sha256 of every file, csHash of every key).
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const snarkjs = require(path.join(__dirname, '..', 'oracle', 'ref_shim.js'));
const OUT = path.join(__dirname, '..', 'tests', 'golden');
const sha = b => crypto.createHash('sha256').update(b).digest('hex');

(async () => {
    const index = {};
    for (const name of ['bn128', 'bls12381']) {
        snarkjs.reseed();
        const curve = await snarkjs.curves.getCurveFromName(name);
        const mem = () => ({ type: 'mem' });
        const p0 = mem(), p1 = mem(), pf = mem();
        await snarkjs.powersOfTau.newAccumulator(curve, 8, p0);
        await snarkjs.powersOfTau.contribute(p0, p1, 'C1', 'Entropy1');
        await snarkjs.powersOfTau.preparePhase2(p1, pf);
        fs.writeFileSync(path.join(OUT, `setup_${name}_p8.ptau`), pf.data);
        index[`setup_${name}_p8.ptau`] = { sha256: sha(pf.data) };
        for (const kind of ['edge', 'full']) {
            const r1cs = new Uint8Array(fs.readFileSync(path.join(OUT, `setup_${name}_${kind}.r1cs`)));
            const z = mem();
            const csHash = await snarkjs.zKey.newZKey(r1cs, pf, z);
            if (csHash === -1) throw new Error(`newZKey refused ${name} ${kind}`);
            fs.writeFileSync(path.join(OUT, `setup_${name}_${kind}.zkey`), z.data);
            index[`setup_${name}_${kind}.r1cs`] = { sha256: sha(r1cs) };
            index[`setup_${name}_${kind}.zkey`] = { sha256: sha(z.data), csHash: Buffer.from(csHash).toString('hex') };
            console.log(name, kind, 'zkey', z.data.length, 'bytes, csHash', Buffer.from(csHash).toString('hex').slice(0, 16));
        }
    }
    fs.writeFileSync(path.join(OUT, 'setup_golden.json'), JSON.stringify(index, null, 1) + '\n');
    process.exit(0);
})().catch(e => { console.error(e); process.exit(1); });
