// tools/gen_phase2_golden.js — golden vectors of the Groth16 phase-2 contribution (snarkjs_amd/groth16_phase2.py, csrc/phase2_host.hip), produced by
// the REFERENCE on the CPU from the keys tools/gen_setup_golden.js wrote:
//   node --harmony-optional-chaining --harmony-nullish tools/gen_phase2_golden.js
// Per curve: setup_<curve>_full.zkey -> contribute('c1', 'Entropy1') -> beacon('b2', 0102..1f, 10) -> contribute(undefined, 'Entropy3') and
// setup_<curve>_edge.zkey -> contribute('c1', 'Entropy1'), written as tests/golden/phase2_<curve>_<key>_<step>.zkey. phase2_golden.json records per key
// its sha256, the contribution hash the call returned, the call's arguments and the 64 bytes contribute drew from getRandomValues; and, per curve, direct
// vectors of the host functions: seed -> (Fr.fromRng, G1.fromRng), transcript -> hashToG2, and the ChaCha seed of the beacon.
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const snarkjs = require(path.join(__dirname, '..', 'oracle', 'ref_shim.js'));
const OUT = path.join(__dirname, '..', 'tests', 'golden');
const sha = b => crypto.createHash('sha256').update(b).digest('hex');
const hex = b => Buffer.from(b).toString('hex');
const BEACON = Array.from({ length: 31 }, (_, i) => (i + 1).toString(16).padStart(2, '0')).join('');

// in browser mode beacon hashes through crypto.subtle.digest, which the shim's crypto object lacks; contribute draws its 64 bytes from getRandomValues
let drawn = [];
const plainRandom = globalThis.crypto.getRandomValues;
globalThis.crypto.getRandomValues = a => { const r = plainRandom(a); if (a.byteLength === 64) drawn.push(hex(new Uint8Array(a.buffer, a.byteOffset, 64))); return r; };
globalThis.crypto.subtle = {
    digest: async (alg, ab) => {
        if (alg !== 'SHA-256') throw new Error('only SHA-256');
        const d = crypto.createHash('sha256').update(Buffer.from(ab)).digest();
        return d.buffer.slice(d.byteOffset, d.byteOffset + d.byteLength);
    },
};

(async () => {
    const files = {}, vectors = {};
    for (const name of ['bn128', 'bls12381']) {
        snarkjs.reseed();
        const curve = await snarkjs.curves.getCurveFromName(name);
        // the generator class behind every fromRng, and the seed a call derived: taken from the object the reference hands to Fr.fromRng
        let ChaCha = null, seedSeen = null;
        const frFromRng = curve.Fr.fromRng;
        curve.Fr.fromRng = function (rng) { ChaCha = rng.constructor; seedSeen = rng.state.slice(4, 12); return frFromRng.call(this, rng); };

        const step = async (from, to, op, args) => {
            const old = { type: 'mem', data: new Uint8Array(fs.readFileSync(path.join(OUT, from))) }, out = { type: 'mem' };
            drawn = [];
            const h = op === 'contribute' ? await snarkjs.zKey.contribute(old, out, args.name, args.entropy) : await snarkjs.zKey.beacon(old, out, args.name, args.beaconHash, args.numIterationsExp);
            if (!h || h === -1) throw new Error(`${op} refused ${from}`);
            if (drawn.length !== (op === 'contribute' ? 1 : 0)) throw new Error(`${op} drew ${drawn.length} x 64 random bytes`);
            fs.writeFileSync(path.join(OUT, to), out.data);
            files[to] = Object.assign({ sha256: sha(out.data), contributionHash: hex(h), from, op, random64: drawn[0] || null, seed: seedSeen }, args);
            console.log(to, out.data.length, 'bytes, contribution hash', hex(h).slice(0, 16));
        };
        await step(`setup_${name}_full.zkey`, `phase2_${name}_full_c1.zkey`, 'contribute', { name: 'c1', entropy: 'Entropy1' });
        await step(`phase2_${name}_full_c1.zkey`, `phase2_${name}_full_b2.zkey`, 'beacon', { name: 'b2', beaconHash: BEACON, numIterationsExp: 10 });
        await step(`phase2_${name}_full_b2.zkey`, `phase2_${name}_full_c3.zkey`, 'contribute', { name: null, entropy: 'Entropy3' });
        await step(`setup_${name}_edge.zkey`, `phase2_${name}_edge_c1.zkey`, 'contribute', { name: 'c1', entropy: 'Entropy1' });
        curve.Fr.fromRng = frFromRng;

        // direct vectors; a counting generator tells which of them needed a rejection in F.fromRng or a second pass of G.fromRng's x loop
        const counted = seed => { const rng = new ChaCha(seed); rng.u64 = 0; rng.bools = 0; const a = rng.nextU64, b = rng.nextBool;
            rng.nextU64 = function () { this.u64++; return a.call(this); }; rng.nextBool = function () { this.bools++; return b.call(this); }; return rng; };
        const v = { fromRng: [], hashToG2: [] };
        let rejections = 0, passes = 0;
        for (let i = 0; i < 24; i++) {
            const seed = Array.from(new Uint32Array(crypto.createHash('sha256').update(`phase2 seed ${name} ${i}`).digest().buffer.slice(0, 32)));
            const rng = counted(seed);
            const fr = curve.Fr.fromRng(rng), frDraws = rng.u64;
            const g1 = curve.G1.toAffine(curve.G1.fromRng(rng));
            if (frDraws > curve.Fr.n64) rejections++;
            if (rng.bools > 1) passes++;
            v.fromRng.push({ seed, fr: hex(fr), g1: hex(g1), frDraws, xPasses: rng.bools });
        }
        for (let i = 0; i < 24; i++) {
            const transcript = crypto.createHash('sha512').update(`phase2 transcript ${name} ${i}`).digest();
            const seed = [];
            for (let k = 0; k < 8; k++) seed.push(transcript.readUInt32BE(4 * k));             // src/keypair.js hashToG2
            const rng = counted(seed);
            const g2 = curve.G2.toAffine(curve.G2.fromRng(rng));
            if (rng.u64 > rng.bools * 2 * curve.F1.n64) rejections++;
            if (rng.bools > 1) passes++;
            v.hashToG2.push({ transcript: hex(transcript), g2: hex(g2), xPasses: rng.bools });
        }
        if (!rejections || !passes) throw new Error(`${name}: no vector needs a rejection (${rejections}) or a second pass (${passes})`);
        v.beaconSeed = { beaconHash: BEACON, numIterationsExp: 10, seed: files[`phase2_${name}_full_b2.zkey`].seed };
        vectors[name] = v;
        console.log(name, 'vectors:', rejections, 'with a rejection,', passes, 'with more than one pass');
    }
    fs.writeFileSync(path.join(OUT, 'phase2_golden.json'), JSON.stringify({ files, vectors }, null, 1) + '\n');
    process.exit(0);
})().catch(e => { console.error(e); process.exit(1); });
