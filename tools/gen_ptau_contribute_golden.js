// tools/gen_ptau_contribute_golden.js — golden files of a phase-1 ceremony (snarkjs_amd/powersoftau_contribute.py, csrc/ptau_contribute.hip), produced by the
// REFERENCE on the CPU:
//   node --harmony-optional-chaining --harmony-nullish tools/gen_ptau_contribute_golden.js
// Per curve a power-1 and a power-5 chain: newAccumulator -> contribute('C1', 'Entropy1') -> contribute('C2', 'Entropy2') -> beacon('B3', 0102..1f, 10), every
// step written as tests/golden/ptau_<curve>_p<power>_{c1,c2,b3}.ptau; the fresh accumulators go in as sha256 only. ptau_contribute_golden.json records per step
// the sha256, the hash the call returned, its arguments, the 64 bytes contribute drew from getRandomValues and the logger's lines (debug lines only for
// newAccumulator); the calls the reference refuses (a reduced file, bad beacon hex, a 256-byte beacon, numIterationsExp 9 and 64) with what they returned or
// threw; what it does at power 0; for BN254 at power 14 (the tauG1 section is two chunks of the response hasher there) the sha256 of both files, the random64
// and section 7 of the contributed file; and vectors for zkmi_blake2b512_partial: the reference's own Blake2b hasher fed the bytes (7 i + 3) & 255 in `update`
// calls of the recorded lengths, and its state as misc.toPartialHash lays it out.
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

function split(raw) {
    const dv = new DataView(raw.buffer, raw.byteOffset, raw.byteLength), out = [];
    let off = 12;
    for (let i = 0; i < dv.getUint32(8, true); i++) {
        const typ = dv.getUint32(off, true), len = Number(dv.getBigUint64(off + 4, true));
        out.push([typ, raw.slice(off + 12, off + 12 + len)]);
        off += 12 + len;
    }
    return out;
}
function join(raw, secs) {
    const parts = [Buffer.from(raw.slice(0, 8)), Buffer.alloc(4)];
    parts[1].writeUInt32LE(secs.length);
    for (const [typ, body] of secs) {
        const h = Buffer.alloc(12);
        h.writeUInt32LE(typ, 0); h.writeBigUInt64LE(BigInt(body.length), 4);
        parts.push(h, Buffer.from(body));
    }
    return new Uint8Array(Buffer.concat(parts));
}
// the rule "truncate4" of the refused cases: header power 4 (the ceremony power stays 5) and the first 2^4-sized prefixes of sections 2 - 5
function truncate4(raw, n8q) {
    const keep = { 2: 31 * 2 * n8q, 3: 16 * 4 * n8q, 4: 16 * 2 * n8q, 5: 16 * 2 * n8q };
    return join(raw, split(raw).map(([typ, body]) => {
        if (typ === 1) { const b = Buffer.from(body); b.writeUInt32LE(4, 4 + n8q); return [typ, new Uint8Array(b)]; }
        return [typ, keep[typ] ? body.slice(0, keep[typ]) : body];
    }));
}

function recorder(withDebug) {
    const lines = [], push = level => text => lines.push([level, text]);
    return { lines, logger: { debug: withDebug ? push('debug') : () => {}, log: push('log'), info: push('info'), warn: push('warn'), error: push('error') } };
}
async function attempt(f) {
    const rec = recorder(false);
    try {
        const r = await f(rec.logger);
        return { returns: r === false ? false : hex(r), lines: rec.lines };
    } catch (e) {
        return { throws: e.message, lines: rec.lines };
    }
}

// The reference's Blake2b class is not among the bundle's exports. Its constructor ASSIGNS this.blockLen on the new object, so while an accessor of that name
// sits on Object.prototype the assignment arrives at its setter with the hasher as `this`; one call that hashes (newAccumulator) hands the class over.
async function blake2bClass(curve) {
    let found = null;
    Object.defineProperty(Object.prototype, 'blockLen', {
        configurable: true, get() { return undefined; },
        set(v) { if (!found && v === 128) found = this; Object.defineProperty(this, 'blockLen', { value: v, writable: true, enumerable: true, configurable: true }); },
    });
    try { await snarkjs.powersOfTau.newAccumulator(curve, 1, { type: 'mem' }); } finally { delete Object.prototype.blockLen; }
    if (!found || !('v0l' in found) || typeof found.update !== 'function') throw new Error('the Blake2b class was not found');
    const B = found.constructor, probe = new B({ dkLen: 64 });
    if (hex(probe.update(new Uint8Array([97, 98, 99])).digest()) !== hex(crypto.createHash('blake2b512').update('abc').digest())) throw new Error('not Blake2b-512');
    return B;
}
function toPartialHash(h) {                       // src/misc.js:111-127
    const res = new Uint8Array(216), w = new Uint32Array(res.buffer, 128, 22);
    res.set(h.buffer);
    ['v0', 'v1', 'v2', 'v3', 'v4', 'v5', 'v6', 'v7'].forEach((k, i) => { w[2 * i] = h[k + 'l']; w[2 * i + 1] = h[k + 'h']; });
    w[18] = h.pos;
    w[16] = h.length - h.pos;
    return res;
}

(async () => {
    const golden = { steps: {}, fresh: {}, refused: [], power0: {}, p14: {}, blake2bPartial: { pattern: '(7 * i + 3) & 255', vectors: [] } };
    for (const name of ['bn128', 'bls12381']) {
        const curve = await snarkjs.curves.getCurveFromName(name);
        const n8q = curve.F1.n8;
        for (const power of [1, 5]) {
            snarkjs.reseed();
            const mem = () => ({ type: 'mem' });
            const a0 = mem(), rec0 = recorder(true);
            const first = await snarkjs.powersOfTau.newAccumulator(curve, power, a0, rec0.logger);
            golden.fresh[`${name}_p${power}`] = { curve: name, power, sha256: sha(a0.data), bytes: a0.data.length, firstChallengeHash: hex(first), lines: rec0.lines };
            let prev = a0, prevName = null;
            for (const [tag, op, args] of [['c1', 'contribute', { name: 'C1', entropy: 'Entropy1' }], ['c2', 'contribute', { name: 'C2', entropy: 'Entropy2' }],
                                           ['b3', 'beacon', { name: 'B3', beaconHash: BEACON, numIterationsExp: 10 }]]) {
                const out = mem(), rec = recorder(false), file = `ptau_${name}_p${power}_${tag}.ptau`;
                drawn = [];
                const h = op === 'contribute' ? await snarkjs.powersOfTau.contribute(prev, out, args.name, args.entropy, rec.logger)
                                              : await snarkjs.powersOfTau.beacon(prev, out, args.name, args.beaconHash, args.numIterationsExp, rec.logger);
                if (!h) throw new Error(`${op} refused ${prevName}`);
                if (drawn.length !== (op === 'contribute' ? 1 : 0)) throw new Error(`${op} drew ${drawn.length} x 64 random bytes`);
                if (out.data.length >= 120 * 1024) throw new Error(`${file} has ${out.data.length} bytes`);
                fs.writeFileSync(path.join(OUT, file), out.data);
                golden.steps[file] = Object.assign({ curve: name, power, sha256: sha(out.data), bytes: out.data.length, returned: hex(h), from: prevName, op, random64: drawn[0] || null, lines: rec.lines }, args);
                console.log(file, out.data.length, 'bytes, response hash', hex(h).slice(0, 16));
                prev = { type: 'mem', data: new Uint8Array(out.data) };
                prevName = file;
            }
            if (!(await snarkjs.powersOfTau.verify(prev))) throw new Error(`the reference does not accept ${prevName}`);
        }
        // ---- what the reference refuses
        const c1 = new Uint8Array(fs.readFileSync(path.join(OUT, `ptau_${name}_p5_c1.ptau`))), reduced = truncate4(c1, n8q);
        const from = `ptau_${name}_p5_c1.ptau`, m = d => ({ type: 'mem', data: new Uint8Array(d) });
        const table = [
            ['contribute into a reduced file', 'contribute', 'truncate4', { name: 'X', entropy: 'e' }],
            ['beacon into a reduced file', 'beacon', 'truncate4', { name: 'X', beaconHash: BEACON, numIterationsExp: 10 }],
            ['beacon hash is not hexadecimal', 'beacon', null, { name: 'X', beaconHash: 'zz', numIterationsExp: 10 }],
            ['beacon hash of odd length', 'beacon', null, { name: 'X', beaconHash: '012', numIterationsExp: 10 }],
            ['beacon hash of 256 bytes', 'beacon', null, { name: 'X', beaconHash: 'ab'.repeat(256), numIterationsExp: 10 }],
            ['numIterationsExp 9', 'beacon', null, { name: 'X', beaconHash: BEACON, numIterationsExp: 9 }],
            ['numIterationsExp 64', 'beacon', null, { name: 'X', beaconHash: BEACON, numIterationsExp: 64 }],
        ];
        for (const [label, op, rule, args] of table) {
            const src = rule ? reduced : c1;
            const r = await attempt(lg => op === 'contribute' ? snarkjs.powersOfTau.contribute(m(src), { type: 'mem' }, args.name, args.entropy, lg)
                                                              : snarkjs.powersOfTau.beacon(m(src), { type: 'mem' }, args.name, args.beaconHash, args.numIterationsExp, lg));
            if (r.returns !== false && r.throws === undefined) throw new Error(`${name}: ${label}: not refused`);
            golden.refused.push(Object.assign({ curve: name, label, op, from, rule }, args, r));
            console.log(name, label, '->', r.throws !== undefined ? `throws ${r.throws}` : r.returns);
        }
        // ---- power 0: section 2 holds one point, so firstPoints[1] is undefined
        const z0 = { type: 'mem' };
        const z = { newAccumulator: await attempt(async lg => { await snarkjs.powersOfTau.newAccumulator(curve, 0, z0, lg); return new Uint8Array(0); }) };
        if (z0.data) {
            z.contribute = await attempt(lg => snarkjs.powersOfTau.contribute(m(z0.data), { type: 'mem' }, 'C1', 'Entropy1', lg));
            z.beacon = await attempt(lg => snarkjs.powersOfTau.beacon(m(z0.data), { type: 'mem' }, 'B1', BEACON, 10, lg));
            z.sha256 = sha(z0.data);
        }
        golden.power0[name] = z;
        console.log(name, 'power 0:', JSON.stringify({ c: z.contribute && (z.contribute.throws || z.contribute.returns), b: z.beacon && (z.beacon.throws || z.beacon.returns) }));
    }
    // ---- BN254 power 14: recorded, not committed
    {
        snarkjs.reseed();
        const curve = await snarkjs.curves.getCurveFromName('bn128');
        const a0 = { type: 'mem' }, a1 = { type: 'mem' };
        await snarkjs.powersOfTau.newAccumulator(curve, 14, a0);
        drawn = [];
        const h = await snarkjs.powersOfTau.contribute(a0, a1, 'C1', 'Entropy1');
        const s7 = split(new Uint8Array(a1.data)).find(([typ]) => typ === 7)[1];
        golden.p14 = { curve: 'bn128', power: 14, freshSha256: sha(a0.data), sha256: sha(a1.data), bytes: a1.data.length, returned: hex(h), name: 'C1', entropy: 'Entropy1', random64: drawn[0], section7: hex(s7) };
        console.log('bn128 power 14:', a1.data.length, 'bytes');
    }
    // ---- the hasher's state after `update` calls of given lengths
    {
        const B = await blake2bClass(await snarkjs.curves.getCurveFromName('bn128'));
        const big = 64 + 524288 + 1000;
        const cuts = [[big], [64, big - 64], [64, 524288, 1000], [64, 524288, 524288, 37], [128], [256], [64, 64], [64, 64 + 128 * 10], [64, 524288 - 64], [127], [129], [64, 63], [64, 65],
                      [64, 128 * 10 + 63], [64, 128 * 10 + 65], [64, 524288 - 65], [64, 524288 - 63], [1], [0], [], [64], [64, 1048544, 1048576], [3, 125, 128, 129]];
        for (const lens of cuts) {
            const h = new B({ dkLen: 64 });
            let at = 0;
            for (const n of lens) {
                const d = new Uint8Array(n);
                for (let i = 0; i < n; i++) d[i] = (7 * (at + i) + 3) & 255;
                h.update(d);
                at += n;
            }
            const partial = toPartialHash(h), digest = h.digest();
            golden.blake2bPartial.vectors.push({ lens, partial: hex(partial), digest: hex(digest) });
        }
        console.log(golden.blake2bPartial.vectors.length, 'partial-hash vectors');
    }
    fs.writeFileSync(path.join(OUT, 'ptau_contribute_golden.json'), JSON.stringify(golden, null, 1) + '\n');
    process.exit(0);
})().catch(e => { console.error(e); process.exit(1); });
