// tools/gen_fflonk_setup_golden.js — golden vectors of the FFLONK setup (snarkjs_amd/fflonk_setup.py, js/fflonk_setup_native.js), produced by the
// REFERENCE on the CPU (BN254): its own fflonk.setup output for
//   tiny, quirks, rows30   against the prepared power-8 ptau of tools/gen_setup_golden.js (511 tauG1 points: domains up to 32),
//   mix, edge              against fflonk_setup_bn128_p12s.ptau, which this script makes: a seeded ceremony at power 12 (new -> contribute), cut to what
//                          fflonk.setup reads at domain 256: the header, the first 9 * 256 + 18 points of section 2, two points of section 3 and an
//                          empty section 12.
// The generator fails when the reference refuses one of them, or accepts one that must be refused: rows31 and setup_bn128_full with either ptau,
// mix and edge with the power-8 ptau. It runs tools/gen_fflonk_setup_r1cs.py first, so the r1cs files on disk are always what
// snarkjs_amd/workloads/synth_r1cs.py builds now (tests/test_fflonk_setup_host.py holds the committed files to the generators as well):
//   node --harmony-optional-chaining --harmony-nullish tools/gen_fflonk_setup_golden.js
// writes tests/golden/fflonk_setup_bn128_{tiny,quirks,rows30,mix,edge}.zkey, fflonk_setup_bn128_p12s.ptau and fflonk_setup_golden.json (sha256 of
// every file, the reference's "Constraints:" and "Additions:" log lines, the refusal texts).
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto'), { execFileSync } = require('child_process');
const snarkjs = require(path.join(__dirname, '..', 'oracle', 'ref_shim.js'));
const OUT = path.join(__dirname, '..', 'tests', 'golden');
const sha = b => crypto.createHash('sha256').update(b).digest('hex');
const read = f => new Uint8Array(fs.readFileSync(path.join(OUT, f)));
const SG1 = 64, SG2 = 128, DOMAIN = 256;

// the sections of a binfile: {type: bytes}
function sections(data) {
    const v = new DataView(data.buffer, data.byteOffset, data.byteLength), out = {};
    let p = 12;
    for (let i = 0; i < v.getUint32(8, true); i++) {
        const type = v.getUint32(p, true), size = Number(v.getBigUint64(p + 4, true));
        out[type] = data.subarray(p + 12, p + 12 + size);
        p += 12 + size;
    }
    return out;
}
function binfile(magic, parts) {
    const chunks = [Buffer.from(magic), Buffer.alloc(8)];
    chunks[1].writeUInt32LE(1, 0); chunks[1].writeUInt32LE(parts.length, 4);
    for (const [type, body] of parts) {
        const h = Buffer.alloc(12);
        h.writeUInt32LE(type, 0); h.writeBigUInt64LE(BigInt(body.length), 4);
        chunks.push(h, Buffer.from(body));
    }
    return new Uint8Array(Buffer.concat(chunks));
}

async function run(r1cs, ptau) {
    const z = { type: 'mem' }, log = [];
    try {
        await snarkjs.fflonk.setup(r1cs, ptau, z, { info: m => log.push(m), error: m => log.push('ERROR ' + m), debug() {}, warn() {} });
    } catch (e) {
        return { refused: e.message };
    }
    const data = z.data instanceof Uint8Array ? z.data : z.data.slice(0, z.data.byteLength);
    return { data, log: log.filter(m => /^\s+(Constraints|Additions):/.test(m)).map(m => m.trim()) };
}

(async () => {
    execFileSync(process.env.PYTHON || 'python', [path.join(__dirname, 'gen_fflonk_setup_r1cs.py')], { stdio: 'inherit' });
    snarkjs.reseed();
    const curve = await snarkjs.curves.getCurveFromName('bn128');
    const p0 = { type: 'mem' }, p1 = { type: 'mem' };
    await snarkjs.powersOfTau.newAccumulator(curve, 12, p0);
    await snarkjs.powersOfTau.contribute(p0, p1, 'C1', 'Entropy1');
    const full = sections(p1.data instanceof Uint8Array ? p1.data : p1.data.slice(0, p1.data.byteLength));
    const p12s = binfile('ptau', [[1, full[1]], [2, full[2].subarray(0, (9 * DOMAIN + 18) * SG1)], [3, full[3].subarray(0, 2 * SG2)], [12, new Uint8Array(0)]]);
    fs.writeFileSync(path.join(OUT, 'fflonk_setup_bn128_p12s.ptau'), p12s);
    const p8 = read('setup_bn128_p8.ptau');
    const index = { 'fflonk_setup_bn128_p12s.ptau': { sha256: sha(p12s) }, 'setup_bn128_p8.ptau': { sha256: sha(p8) } };
    const ptaus = { 'setup_bn128_p8.ptau': p8, 'fflonk_setup_bn128_p12s.ptau': p12s };

    const keys = [['tiny', 'plonk_setup_bn128_tiny.r1cs', 'setup_bn128_p8.ptau'], ['quirks', 'fflonk_setup_bn128_quirks.r1cs', 'setup_bn128_p8.ptau'],
        ['rows30', 'fflonk_setup_bn128_rows30.r1cs', 'setup_bn128_p8.ptau'], ['mix', 'plonk_setup_bn128_mix.r1cs', 'fflonk_setup_bn128_p12s.ptau'],
        ['edge', 'setup_bn128_edge.r1cs', 'fflonk_setup_bn128_p12s.ptau']];
    for (const [kind, file, ptau] of keys) {
        const r1cs = read(file), res = await run(r1cs, ptaus[ptau]);
        if (res.refused) throw new Error(`fflonk.setup refused ${kind}: ${res.refused}`);
        fs.writeFileSync(path.join(OUT, `fflonk_setup_bn128_${kind}.zkey`), res.data);
        index[file] = { sha256: sha(r1cs) };
        index[`fflonk_setup_bn128_${kind}.zkey`] = { sha256: sha(res.data), r1cs: file, ptau, log: res.log };
        console.log(kind, 'zkey', res.data.length, 'bytes', res.log.join(' | '));
    }
    const refusals = [['fflonk_setup_bn128_rows31.r1cs', 'setup_bn128_p8.ptau'], ['plonk_setup_bn128_mix.r1cs', 'setup_bn128_p8.ptau'], ['setup_bn128_edge.r1cs', 'setup_bn128_p8.ptau'],
        ['setup_bn128_full.r1cs', 'setup_bn128_p8.ptau'], ['setup_bn128_full.r1cs', 'fflonk_setup_bn128_p12s.ptau']];
    index.refused = [];
    for (const [file, ptau] of refusals) {
        const r1cs = read(file), res = await run(r1cs, ptaus[ptau]);
        if (!res.refused) throw new Error(`fflonk.setup accepted ${file} with ${ptau}`);
        index[file] = { sha256: sha(r1cs) };
        index.refused.push({ r1cs: file, ptau, message: res.refused });
        console.log(file, ptau, 'refused:', res.refused);
    }
    fs.writeFileSync(path.join(OUT, 'fflonk_setup_golden.json'), JSON.stringify(index, null, 1) + '\n');
    process.exit(0);
})().catch(e => { console.error(e); process.exit(1); });
