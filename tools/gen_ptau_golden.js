// tools/gen_ptau_golden.js — golden files and verdicts of powersOfTau.verify (snarkjs_amd/powersoftau_verify.py), produced by the REFERENCE on the CPU:
//   node --harmony-optional-chaining --harmony-nullish tools/gen_ptau_golden.js
// Per curve a power-6 ceremony: newAccumulator -> contribute('C1') -> contribute('C2') -> beacon('B3', 0102..1f, 10) -> preparePhase2, written as
// tests/golden/ptau_<curve>_p6_c3b_raw.ptau (before preparePhase2) and ptau_<curve>_p6_c3b.ptau. ptau_verify_golden.json records the sha256 of each file and,
// per CASE, what the reference's powersOfTau.verify returned or threw and its info / warn / error lines. A case is a fixture, an optional rule ("truncate4":
// header power 4, prefixes of sections 2 - 5 and 12 - 15) and a list of patches {section, offset, hex} or {section, replace: hex}, applied to the section
// bodies in that order; tests apply the same edits. The reference's verdict for every case is asserted to be the expected one before anything is written.
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const snarkjs = require(path.join(__dirname, '..', 'oracle', 'ref_shim.js'));
const OUT = path.join(__dirname, '..', 'tests', 'golden');
const sha = b => crypto.createHash('sha256').update(b).digest('hex');
const hex = b => Buffer.from(b).toString('hex');
const BEACON = Array.from({ length: 31 }, (_, i) => (i + 1).toString(16).padStart(2, '0')).join('');

// in browser mode beacon hashes through crypto.subtle.digest, which the shim's crypto object lacks
globalThis.crypto.subtle = {
    digest: async (alg, ab) => {
        if (alg !== 'SHA-256') throw new Error('only SHA-256');
        const d = crypto.createHash('sha256').update(Buffer.from(ab)).digest();
        return d.buffer.slice(d.byteOffset, d.byteOffset + d.byteLength);
    },
};

// ---- a file taken apart and put together again
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
function truncate4(raw, n8q) {
    const keep = { 2: 31 * 2 * n8q, 3: 16 * 4 * n8q, 4: 16 * 2 * n8q, 5: 16 * 2 * n8q, 12: 63 * 2 * n8q, 13: 31 * 4 * n8q, 14: 31 * 2 * n8q, 15: 31 * 2 * n8q };
    return join(raw, split(raw).map(([typ, body]) => {
        if (typ === 1) { const b = Buffer.from(body); b.writeUInt32LE(4, 4 + n8q); return [typ, new Uint8Array(b)]; }
        return [typ, keep[typ] ? body.slice(0, keep[typ]) : body];
    }));
}
function applyCase(raw, c, n8q) {
    if (c.rule === 'truncate4') raw = truncate4(raw, n8q);
    for (const p of c.patches || []) {
        raw = join(raw, split(raw).map(([typ, body]) => {
            if (typ !== p.section) return [typ, body];
            if (p.replace !== undefined) return [typ, new Uint8Array(Buffer.from(p.replace, 'hex'))];
            const b = Buffer.from(body);
            Buffer.from(p.hex, 'hex').copy(b, p.offset);
            return [typ, new Uint8Array(b)];
        }));
    }
    return raw;
}
// offsets of the contributions of section 7 and of their fields
function contributions(body, n8q) {
    const s1 = 2 * n8q, s2 = 4 * n8q, dv = new DataView(body.buffer, body.byteOffset, body.byteLength), out = [];
    let o = 4;
    for (let i = 0; i < dv.getUint32(0, true); i++) {
        const c = { at: o, tauG1: o, tauG2: o + s1, alphaG1: o + s1 + s2, betaG1: o + 2 * s1 + s2, betaG2: o + 3 * s1 + s2 };
        c.key = o + 3 * s1 + 2 * s2;
        c.tau_g2_spx = c.key + 6 * s1;
        c.nextChallenge = c.key + 6 * s1 + 3 * s2 + 216;
        c.params = c.nextChallenge + 64 + 8;
        o = c.params + dv.getUint32(c.params - 4, true);
        out.push(c);
    }
    return out;
}

async function run(raw) {
    const lines = [], push = level => text => lines.push([level, text]);
    const logger = { debug: () => {}, info: push('info'), warn: push('warn'), error: push('error') };
    try {
        const verdict = await snarkjs.powersOfTau.verify({ type: 'mem', data: raw }, logger);
        return { verdict, lines };
    } catch (e) {
        return { throws: e.message, lines };
    }
}

(async () => {
    const files = {}, cases = [];
    for (const name of ['bn128', 'bls12381']) {
        snarkjs.reseed();
        const curve = await snarkjs.curves.getCurveFromName(name);
        const n8q = curve.F1.n8, s1 = 2 * n8q, s2 = 4 * n8q;
        const mem = () => ({ type: 'mem' });
        const a0 = mem(), a1 = mem(), a2 = mem(), a3 = mem(), a4 = mem();
        await snarkjs.powersOfTau.newAccumulator(curve, 6, a0);
        await snarkjs.powersOfTau.contribute(a0, a1, 'C1', 'Entropy1');
        await snarkjs.powersOfTau.contribute(a1, a2, 'C2', 'Entropy2');
        await snarkjs.powersOfTau.beacon(a2, a3, 'B3', BEACON, 10);
        await snarkjs.powersOfTau.preparePhase2(a3, a4);
        const fresh = new Uint8Array(a0.data), rawName = `ptau_${name}_p6_c3b_raw.ptau`, prepName = `ptau_${name}_p6_c3b.ptau`;
        for (const [f, d] of [[rawName, a3.data], [prepName, a4.data]]) {
            if (d.length >= 120 * 1024) throw new Error(`${f} has ${d.length} bytes`);
            fs.writeFileSync(path.join(OUT, f), d);
            files[f] = { sha256: sha(d), bytes: d.length };
        }
        const prep = new Uint8Array(a4.data), secs = new Map(split(prep)), cs = contributions(secs.get(7), n8q), last = cs[2], s7 = secs.get(7);
        const at = (o, n) => hex(s7.slice(o, o + n));
        const swap = (section, size, i, j, base) => [{ section, offset: (base + i) * size, hex: hex(secs.get(section).slice((base + j) * size, (base + j + 1) * size)) },
                                                     { section, offset: (base + j) * size, hex: hex(secs.get(section).slice((base + i) * size, (base + i + 1) * size)) }];
        const flip = (o) => [{ section: 7, offset: o, hex: hex([s7[o] ^ 1]) }];
        const times3 = Buffer.concat(Array.from({ length: 64 }, (_, i) => {
            const b = new Uint8Array(s1);
            curve.G1.toRprLEM(b, 0, curve.G1.timesScalar(curve.G1.fromRprLEM(secs.get(4), i * s1), 3));
            return Buffer.from(b);
        }));
        const g2gen = new Uint8Array(s2);
        curve.G2.toRprLEM(g2gen, 0, curve.G2.g);
        const none = Buffer.alloc(4);
        const table = [
            ['p8 unpatched', `setup_${name}_p8.ptau`, {}, true],
            ['p6 prepared unpatched', prepName, {}, true],
            ['p6 raw unpatched', rawName, {}, true],
            ['truncated to power 4', prepName, { rule: 'truncate4' }, true],
            ['truncated, a nextChallenge byte flipped', prepName, { rule: 'truncate4', patches: flip(last.nextChallenge + 9) }, true],
            ['no contributions', prepName, { patches: [{ section: 7, replace: hex(none) }] }, false],
            ['last tau.g2_spx <- betaG2', prepName, { patches: [{ section: 7, offset: last.tau_g2_spx, hex: at(last.betaG2, s2) }] }, false],
            ['contribution 2 tau.g2_spx <- betaG2', prepName, { patches: [{ section: 7, offset: cs[1].tau_g2_spx, hex: at(cs[1].betaG2, s2) }] }, false],
            ['last tauG1 <- alphaG1', prepName, { patches: [{ section: 7, offset: last.tauG1, hex: at(last.alphaG1, s1) }] }, false],
            ['contribution 1 betaG1 <- alphaG1', prepName, { patches: [{ section: 7, offset: cs[0].betaG1, hex: at(cs[0].alphaG1, s1) }] }, false],
            ['beacon iterations 10 -> 11', prepName, { patches: [{ section: 7, offset: last.params + 2 + 2 + 1, hex: '0b' }] }, false],
            ['tauG1 points 3 and 5 swapped', prepName, { patches: swap(2, s1, 3, 5, 0) }, false],
            ['tauG2 points 3 and 5 swapped', prepName, { patches: swap(3, s2, 3, 5, 0) }, false],
            ['alphaTauG1 times 3', prepName, { patches: [{ section: 4, replace: hex(times3) }] }, false],
            ['betaG2 section <- the generator', prepName, { patches: [{ section: 6, replace: hex(g2gen) }] }, false],
            ['a nextChallenge byte flipped', prepName, { patches: flip(last.nextChallenge + 9) }, false],
            ['two points of the top block of section 12 swapped', prepName, { patches: swap(12, s1, 3, 5, 127) }, false],
            ['two points of the top block of section 13 swapped', prepName, { patches: swap(13, s2, 3, 5, 63) }, false],
            ['a Groth16 zkey', `groth16_${name}_n1024.zkey`, {}, 'throws'],
        ];
        if (s7[last.params + 4] !== 2 || s7[last.params + 5] !== 10) throw new Error('the beacon parameters are not where the patch expects them');
        for (const [label, fixture, c, expect] of table) {
            const raw = applyCase(new Uint8Array(fs.readFileSync(path.join(OUT, fixture))), c, n8q);
            const r = await run(raw);
            if (expect === 'throws' ? r.throws === undefined : r.verdict !== expect) throw new Error(`${name}: ${label}: expected ${expect}, got ${JSON.stringify(r)}`);
            cases.push(Object.assign({ curve: name, label, fixture }, c, r));
            console.log(name, label, '->', r.throws !== undefined ? `throws ${r.throws}` : r.verdict, r.lines.length ? r.lines[r.lines.length - 1][1].split('\n')[0] : '');
        }
        const f = await run(fresh);
        if (f.verdict !== false || f.lines.length !== 1 || f.lines[0][1] !== 'This file has no contribution! It cannot be used in production') throw new Error('fresh accumulator: ' + JSON.stringify(f));
    }
    fs.writeFileSync(path.join(OUT, 'ptau_verify_golden.json'), JSON.stringify({ files, cases }, null, 1) + '\n');
    process.exit(0);
})().catch(e => { console.error(e); process.exit(1); });
