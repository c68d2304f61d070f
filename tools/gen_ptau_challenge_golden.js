// tools/gen_ptau_challenge_golden.js — golden files of the challenge / response round trip of phase 1 (snarkjs_amd/powersoftau_challenge.py,
// csrc/ptau_challenge.hip), produced by the REFERENCE on the CPU:
//   node --harmony-optional-chaining --harmony-nullish tools/gen_ptau_challenge_golden.js
// Per curve, at power 1 and power 5, from the committed tests/golden/ptau_<curve>_p<power>_c1.ptau: exportChallenge -> challengeContribute('Entropy2') ->
// importResponse('C2', with points) and importResponse('C2', without points), written as ptau_<curve>_p<power>_c1.challenge, .response, _imported.ptau and
// _imported_nopoints.ptau. ptau_challenge_golden.json records per step the sha256, what the call returned, the 64 bytes challengeContribute drew from
// getRandomValues and the logger's info / error lines; the calls the reference refuses or dies in (export from a file imported without points, a challenge
// of a wrong size, a response of a wrong size, a response to another challenge, a file whose points are not the declared ones) with what they threw; a second
// response imported onto the file without points (the 0xFF x 64 hash adopts the response's previous hash); and what it does at power 0.
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const snarkjs = require(path.join(__dirname, '..', 'oracle', 'ref_shim.js'));
const OUT = path.join(__dirname, '..', 'tests', 'golden');
const sha = b => crypto.createHash('sha256').update(b).digest('hex');
const hex = b => Buffer.from(b).toString('hex');

let drawn = [];
const plainRandom = globalThis.crypto.getRandomValues;
globalThis.crypto.getRandomValues = a => { const r = plainRandom(a); if (a.byteLength === 64) drawn.push(hex(new Uint8Array(a.buffer, a.byteOffset, 64))); return r; };

function recorder() {
    const lines = [], push = level => text => lines.push([level, text]);
    return { lines, logger: { debug: () => {}, log: push('log'), info: push('info'), warn: push('warn'), error: push('error') } };
}
async function attempt(f) {
    const rec = recorder();
    try {
        const r = await f(rec.logger);
        return { returns: r === undefined ? null : hex(r), lines: rec.lines };
    } catch (e) {
        return { throws: e.message, lines: rec.lines };
    }
}
const m = d => ({ type: 'mem', data: new Uint8Array(d) });
const mem = () => ({ type: 'mem' });

(async () => {
    const golden = { trips: {}, refused: [], second: {}, power0: {} };
    const P = snarkjs.powersOfTau;
    for (const name of ['bn128', 'bls12381']) {
        const curve = await snarkjs.curves.getCurveFromName(name);
        let last = null;
        for (const power of [1, 5]) {
            snarkjs.reseed();
            const from = `ptau_${name}_p${power}_c1.ptau`, stem = `ptau_${name}_p${power}_c1`;
            const old = new Uint8Array(fs.readFileSync(path.join(OUT, from)));
            const ch = mem(), rs = mem(), full = mem(), bare = mem();
            const r1 = recorder(), r2 = recorder(), r3 = recorder(), r4 = recorder();
            const challengeHash = await P.exportChallenge(m(old), ch, r1.logger);
            drawn = [];
            await P.challengeContribute(curve, m(ch.data), rs, 'Entropy2', r2.logger);
            if (drawn.length !== 1) throw new Error(`challengeContribute drew ${drawn.length} x 64 random bytes`);
            const next = await P.importResponse(m(old), m(rs.data), full, 'C2', true, r3.logger);
            const none = await P.importResponse(m(old), m(rs.data), bare, 'C2', false, r4.logger);
            if (!(await P.verify(m(full.data)))) throw new Error(`the reference does not accept the import of ${from}`);
            const files = { challenge: [`${stem}.challenge`, ch.data], response: [`${stem}.response`, rs.data], imported: [`${stem}_imported.ptau`, full.data],
                            nopoints: [`${stem}_imported_nopoints.ptau`, bare.data] };
            const rec = { curve: name, power, from, entropy: 'Entropy2', name: 'C2', random64: drawn[0], challengeHash: hex(challengeHash), nextChallenge: hex(next), noPointsReturned: hex(none),
                          lines: { exportChallenge: r1.lines, challengeContribute: r2.lines, importResponse: r3.lines, importResponseNoPoints: r4.lines }, files: {} };
            for (const [k, [file, data]] of Object.entries(files)) {
                if (data.length >= 120 * 1024) throw new Error(`${file} has ${data.length} bytes`);
                fs.writeFileSync(path.join(OUT, file), data);
                rec.files[k] = { file, sha256: sha(data), bytes: data.length };
            }
            golden.trips[`${name}_p${power}`] = rec;
            console.log(stem, Object.values(rec.files).map(f => f.bytes).join(' / '), 'bytes');
            last = { old, ch: ch.data, rs: rs.data, full: full.data, bare: bare.data, power };
        }
        // ---- a second response, imported onto the file with points and onto the one without (recorded, not committed)
        {
            const ch = mem(), rs = mem(), a = mem(), b = mem();
            await P.exportChallenge(m(last.full), ch);
            drawn = [];
            await P.challengeContribute(curve, m(ch.data), rs, 'Entropy3');
            const ra = await attempt(lg => P.importResponse(m(last.full), m(rs.data), a, 'C3', true, lg));
            const rb = await attempt(lg => P.importResponse(m(last.bare), m(rs.data), b, 'C3', true, lg));
            golden.second[name] = { power: last.power, entropy: 'Entropy3', name: 'C3', random64: drawn[0], responseSha256: sha(rs.data), ontoFull: Object.assign(ra, { sha256: a.data && sha(a.data) }),
                                    ontoNoPoints: Object.assign(rb, { sha256: b.data && sha(b.data) }) };
        }
        // ---- what the reference refuses or dies in (power 5)
        const other = new Uint8Array(fs.readFileSync(path.join(OUT, `ptau_${name}_p1_c1.ptau`)));
        const broken = new Uint8Array(last.old);
        {   // the first point of section 2 := the second: still on the curve, no longer the declared file
            const dv = new DataView(broken.buffer);
            let off = 12, at = -1;
            for (let i = 0; i < dv.getUint32(8, true); i++) { const typ = dv.getUint32(off, true), len = Number(dv.getBigUint64(off + 4, true)); if (typ === 2) at = off + 12; off += 12 + len; }
            const sG1 = curve.F1.n8 * 2;
            broken.set(broken.slice(at + sG1, at + 2 * sG1), at);
        }
        const longer = new Uint8Array(last.ch.length + 1), longerR = new Uint8Array(last.rs.length + 1);
        longer.set(last.ch); longerR.set(last.rs);
        const table = [
            ['export from a file imported without points', lg => P.exportChallenge(m(last.bare), mem(), lg)],
            ['export from a file whose points are not the declared ones', lg => P.exportChallenge(m(broken), mem(), lg)],
            ['a challenge one byte longer', lg => P.challengeContribute(curve, m(longer), mem(), 'e', lg)],
            ['a challenge one byte shorter', lg => P.challengeContribute(curve, m(last.ch.slice(0, -1)), mem(), 'e', lg)],
            ['a response one byte longer', lg => P.importResponse(m(last.old), m(longerR), mem(), 'x', true, lg)],
            ['a response of another power', lg => P.importResponse(m(other), m(last.rs), mem(), 'x', true, lg)],
            ['a response to another challenge', lg => P.importResponse(m(last.full), m(last.rs), mem(), 'x', true, lg)],
        ];
        for (const [label, f] of table) {
            const r = await attempt(f);
            if (r.throws === undefined) throw new Error(`${name}: ${label}: not refused`);
            golden.refused.push(Object.assign({ curve: name, label }, r));
            console.log(name, label, '-> throws', r.throws);
        }
        // ---- power 0
        {
            const z0 = mem(), ch = mem(), rs = mem();
            await P.newAccumulator(curve, 0, z0);
            const z = { exportChallenge: await attempt(lg => P.exportChallenge(m(z0.data), ch, lg)) };
            if (ch.data) {
                z.challengeBytes = ch.data.length;
                z.challengeContribute = await attempt(lg => P.challengeContribute(curve, m(ch.data), rs, 'Entropy1', lg));
                if (rs.data) {
                    z.responseBytes = rs.data.length;
                    z.importResponse = await attempt(lg => P.importResponse(m(z0.data), m(rs.data), mem(), 'C1', true, lg));
                    z.importResponseNoPoints = await attempt(lg => P.importResponse(m(z0.data), m(rs.data), mem(), 'C1', false, lg));
                }
            }
            golden.power0[name] = z;
            console.log(name, 'power 0:', JSON.stringify(Object.fromEntries(Object.entries(z).filter(([, v]) => v && typeof v === 'object').map(([k, v]) => [k, v.throws || 'ok']))));
        }
    }
    fs.writeFileSync(path.join(OUT, 'ptau_challenge_golden.json'), JSON.stringify(golden, null, 1) + '\n');
    process.exit(0);
})().catch(e => { console.error(e); process.exit(1); });
