// tools/gen_bellman_golden.js — golden vectors of the Bellman phase-2 round trip (snarkjs_amd/groth16_bellman.py, csrc/bellman.hip), produced by the
// REFERENCE on the CPU from the keys tools/gen_phase2_golden.js wrote:
//   node --harmony-optional-chaining --harmony-nullish tools/gen_bellman_golden.js
// Per curve and per circuit (full: domain 256, 60 variables; edge: domain 128, 12 variables, points at infinity in L, A and B1):
//   phase2_<curve>_<circuit>_c1.zkey -> exportBellman -> tests/golden/bellman_<curve>_<circuit>_challenge.params
//   -> bellmanContribute(curve, ..., 'EntropyB') -> tests/golden/bellman_<curve>_<circuit>_response.params
//   -> importBellman(c1, response, 'imp'): recorded in bellman_golden.json by the sha256 of the key and of each of its sections, with the reference's verdict
//      of verifyFromInit on it.
// bellman_golden.json also records the sha256 of every file, the contribution hash, the 64 bytes bellmanContribute drew from getRandomValues, and what the
// reference returned or threw for the refused cases.
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const snarkjs = require(path.join(__dirname, '..', 'oracle', 'ref_shim.js'));
const OUT = path.join(__dirname, '..', 'tests', 'golden');
const sha = b => crypto.createHash('sha256').update(b).digest('hex');
const hex = b => Buffer.from(b).toString('hex');
const mem = b => ({ type: 'mem', data: new Uint8Array(b) });
const gold = f => mem(fs.readFileSync(path.join(OUT, f)));

let drawn = [];
const plainRandom = globalThis.crypto.getRandomValues;
globalThis.crypto.getRandomValues = a => { const r = plainRandom(a); if (a.byteLength === 64) drawn.push(hex(new Uint8Array(a.buffer, a.byteOffset, 64))); return r; };

// sha256 of each section of a binfile, in the order the file holds them
function sections(data) {
    const b = Buffer.from(data), out = [];
    let o = 12;
    for (let i = 0; i < b.readUInt32LE(8); i++) {
        const type = b.readUInt32LE(o), size = Number(b.readBigUInt64LE(o + 4));
        out.push({ type, size, sha256: sha(b.slice(o + 12, o + 12 + size)) });
        o += 12 + size;
    }
    return out;
}
// one call the reference refuses: what it returned or threw, and the lines it logged
async function refused(fn) {
    const lines = [], logger = { info: s => lines.push(['info', s]), error: s => lines.push(['error', s]), debug: () => {}, warn: s => lines.push(['warn', s]) };
    try { return { returned: await fn(logger), lines }; } catch (e) { return { threw: e.message, lines }; }
}

(async () => {
    const files = {}, imported = {}, refusals = {};
    for (const name of ['bn128', 'bls12381']) {
        snarkjs.reseed();
        const curve = await snarkjs.curves.getCurveFromName(name);
        for (const circuit of ['full', 'edge']) {
            const key = `phase2_${name}_${circuit}_c1.zkey`, chName = `bellman_${name}_${circuit}_challenge.params`, rsName = `bellman_${name}_${circuit}_response.params`;
            const ch = { type: 'mem' }, rs = { type: 'mem' }, nw = { type: 'mem' };
            await snarkjs.zKey.exportBellman(gold(key), ch);
            fs.writeFileSync(path.join(OUT, chName), ch.data);
            files[chName] = { sha256: sha(ch.data), from: key, op: 'exportBellman' };
            drawn = [];
            const h = await snarkjs.zKey.bellmanContribute(curve, mem(ch.data), rs, 'EntropyB');
            if (drawn.length !== 1) throw new Error(`bellmanContribute drew ${drawn.length} x 64 random bytes`);
            fs.writeFileSync(path.join(OUT, rsName), rs.data);
            files[rsName] = { sha256: sha(rs.data), from: chName, op: 'bellmanContribute', entropy: 'EntropyB', random64: drawn[0], contributionHash: hex(h) };
            const ok = await snarkjs.zKey.importBellman(gold(key), mem(rs.data), nw, 'imp');
            if (ok !== true) throw new Error(`importBellman refused ${rsName}`);
            const verdict = await snarkjs.zKey.verifyFromInit(gold(`setup_${name}_${circuit}.zkey`), gold(`setup_${name}_p8.ptau`), mem(nw.data));
            imported[`${name}_${circuit}`] = { old: key, params: rsName, name: 'imp', sha256: sha(nw.data), bytes: nw.data.length, sections: sections(nw.data), verifyFromInit: verdict };
            console.log(name, circuit, ch.data.length, rs.data.length, nw.data.length, 'bytes; verifyFromInit', verdict);
        }
        // the refused cases, on the full circuit
        const key = `phase2_${name}_full_c1.zkey`, rs = fs.readFileSync(path.join(OUT, `bellman_${name}_full_response.params`));
        const hdr = (await snarkjs.zKey.exportJson(gold(key)));
        const sG1 = curve.G1.F.n8 * 2, sG2 = curve.G2.F.n8 * 2;
        const atH = 3 * sG1 + 3 * sG2 + 4 + sG1 * (hdr.nPublic + 1);
        const atContributions = 3 * sG1 + 3 * sG2 + 8 + sG1 * hdr.nVars + 4 + sG1 * (hdr.domainSize - 1) + 4 + sG1 * hdr.nVars + 4 + sG1 * hdr.nVars + 4 + sG2 * hdr.nVars + 64 + 4;
        const flipped = Buffer.from(rs), wrongH = Buffer.from(rs);
        flipped[atContributions + 3 * sG1 + sG2 + 5] ^= 1;                      // inside the transcript of contribution 0
        wrongH.writeUInt32BE(hdr.domainSize, atH);
        const r = {};
        r.plonk_export = await refused(l => snarkjs.zKey.exportBellman(gold('plonk_bn128_small.zkey'), { type: 'mem' }, l));
        r.plonk_import = await refused(l => snarkjs.zKey.importBellman(gold('plonk_bn128_small.zkey'), mem(rs), { type: 'mem' }, 'x', l));
        r.fewer_contributions = Object.assign({ old: `phase2_${name}_full_c3.zkey` }, await refused(l => snarkjs.zKey.importBellman(gold(`phase2_${name}_full_c3.zkey`), mem(rs), { type: 'mem' }, 'x', l)));
        r.flipped_transcript = Object.assign({ at: atContributions + 3 * sG1 + sG2 + 5 }, await refused(l => snarkjs.zKey.importBellman(gold(key), mem(flipped), { type: 'mem' }, 'x', l)));
        r.wrong_h_count = Object.assign({ at: atH, value: hdr.domainSize }, await refused(l => snarkjs.zKey.importBellman(gold(key), mem(wrongH), { type: 'mem' }, 'x', l)));
        r.cut_by_10 = await refused(l => snarkjs.zKey.importBellman(gold(key), mem(rs.slice(0, rs.length - 10)), { type: 'mem' }, 'x', l));
        refusals[name] = r;
        for (const k of Object.keys(r)) console.log(name, k, JSON.stringify(r[k].returned), r[k].threw || '', JSON.stringify(r[k].lines));
    }
    fs.writeFileSync(path.join(OUT, 'bellman_golden.json'), JSON.stringify({ files, imported, refusals }, null, 1) + '\n');
    process.exit(0);
})().catch(e => { console.error(e); process.exit(1); });
