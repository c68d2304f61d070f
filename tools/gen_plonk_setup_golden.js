// tools/gen_plonk_setup_golden.js — golden vectors of the PLONK setup (snarkjs_amd/plonk_setup.py, js/plonk_setup_native.js), produced by the
// REFERENCE on the CPU: its own plonk.setup output for the existing setup_<curve>_edge.r1cs and for the mix and tiny fixtures that
// tools/gen_plonk_setup_r1cs.py writes, all against the prepared power-8 ptau of tools/gen_setup_golden.js. The generator fails when the reference
// refuses one of them (a mix circuit of more than 256 PLONK rows); setup_<curve>_full.r1cs must be refused (it does not fit power 8 under PLONK).
// It runs tools/gen_plonk_setup_r1cs.py first, so the r1cs files on disk are always what snarkjs_amd/workloads/synth_r1cs.py builds now (the
// generators are seeded; tests/test_plonk_setup_host.py holds the committed files to them as well):
//   node --harmony-optional-chaining --harmony-nullish tools/gen_plonk_setup_golden.js
// writes tests/golden/plonk_setup_<curve>_{edge,mix,tiny}.zkey and plonk_setup_golden.json (sha256 of every file, the refusal text of the full circuit).
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto'), { execFileSync } = require('child_process');
const snarkjs = require(path.join(__dirname, '..', 'oracle', 'ref_shim.js'));
const OUT = path.join(__dirname, '..', 'tests', 'golden');
const sha = b => crypto.createHash('sha256').update(b).digest('hex');

(async () => {
    execFileSync(process.env.PYTHON || 'python', [path.join(__dirname, 'gen_plonk_setup_r1cs.py')], { stdio: 'inherit' });
    const index = {};
    for (const name of ['bn128', 'bls12381']) {
        const ptau = new Uint8Array(fs.readFileSync(path.join(OUT, `setup_${name}_p8.ptau`)));
        for (const [kind, file] of [['edge', `setup_${name}_edge.r1cs`], ['mix', `plonk_setup_${name}_mix.r1cs`], ['tiny', `plonk_setup_${name}_tiny.r1cs`]]) {
            const r1cs = new Uint8Array(fs.readFileSync(path.join(OUT, file)));
            const z = { type: 'mem' }, log = [];
            const rc = await snarkjs.plonk.setup(r1cs, ptau, z, { info: m => log.push(m), error: m => log.push('ERROR ' + m), debug() {} });
            if (rc === -1) throw new Error(`plonk.setup refused ${name} ${kind}: ${log.join(' | ')}`);
            const data = z.data instanceof Uint8Array ? z.data : z.data.slice(0, z.data.byteLength);
            fs.writeFileSync(path.join(OUT, `plonk_setup_${name}_${kind}.zkey`), data);
            index[file] = { sha256: sha(r1cs) };
            index[`plonk_setup_${name}_${kind}.zkey`] = { sha256: sha(data), log: log.filter(m => m.startsWith('Plonk constraints')) };
            console.log(name, kind, 'zkey', data.length, 'bytes', log.join(' | '));
        }
        const errs = [];
        const rc = await snarkjs.plonk.setup(new Uint8Array(fs.readFileSync(path.join(OUT, `setup_${name}_full.r1cs`))), ptau, { type: 'mem' }, { info() {}, error: m => errs.push(m), debug() {} });
        if (rc !== -1) throw new Error(`plonk.setup accepted ${name} full`);
        index[`setup_${name}_full.r1cs`] = { refused: errs[0] };
        console.log(name, 'full refused:', errs[0]);
    }
    fs.writeFileSync(path.join(OUT, 'plonk_setup_golden.json'), JSON.stringify(index, null, 1) + '\n');
    process.exit(0);
})().catch(e => { console.error(e); process.exit(1); });
