// tests/js/ptau_verify_lib.js — shared by ptau_verify_cpu.js and ptau_verify_gpu.js: the cases of tests/golden/ptau_verify_golden.json with their rule and
// patches applied (the edits tools/gen_ptau_golden.js made), a powersOfTau.verify call with its info / warn / error lines captured, and the device calls of
// js/powersoftau_verify_native.js restated on the reference's own curve object (its batchLEMtoU, multiExpAffine, fft and pairingEq, power by power as
// verifyLagrangeEvaluations writes them) with the scalars of the library's sequential generator on the host.
"use strict";
const fs = require("fs"), path = require("path");
const P2 = require("./phase2_verify_lib.js");
const ROOT = P2.ROOT;
const INDEX = JSON.parse(fs.readFileSync(path.join(ROOT, "tests", "golden", "ptau_verify_golden.json"), "utf8"));

function truncate4(raw, n8q) {
    const keep = { 2: 31 * 2 * n8q, 3: 16 * 4 * n8q, 4: 16 * 2 * n8q, 5: 16 * 2 * n8q, 12: 63 * 2 * n8q, 13: 31 * 4 * n8q, 14: 31 * 2 * n8q, 15: 31 * 2 * n8q };
    return P2.join(raw, P2.split(raw).map(([t, b]) => {
        if (t === 1) { const o = Buffer.from(b); o.writeUInt32LE(4, 4 + n8q); return [t, new Uint8Array(o)]; }
        return [t, keep[t] ? b.subarray(0, keep[t]) : b];
    }));
}
function caseFile(c, n8q) {
    let raw = P2.G(c.fixture);
    if (c.rule === "truncate4") raw = truncate4(raw, n8q);
    for (const p of c.patches || [])
        raw = P2.withSection(raw, p.section, (b) => {
            if (p.replace !== undefined) return new Uint8Array(Buffer.from(p.replace, "hex"));
            const o = Uint8Array.from(b);
            o.set(Buffer.from(p.hex, "hex"), p.offset);
            return o;
        });
    return raw;
}
// run f(logger): { result | error, lines } with the debug lines left out
async function capture(f) {
    const r = await P2.capture(f);
    r.lines = r.lines.filter((x) => x[0] !== "debug");
    return r;
}
// what follows the file's name in a thrown message (the reference puts fd.fileName in front, "[object Object]" for a file in memory)
const afterName = (m) => (m === undefined ? m : m.replace(/^[^:]*: /, "").trim());

function refDevice(curve, cv, addon, base) {
    const seedWords = (b32) => { const w = new Uint32Array(8), b = Buffer.from(b32.buffer, b32.byteOffset, 32); for (let i = 0; i < 8; i++) w[i] = b.readUInt32BE(4 * i); return w; };
    const words = (seed32, n) => { const s = new Uint8Array(4 * Math.max(n, 1)); addon.call("zkmi_chacha_struct_words_host", seedWords(seed32), 0, s, n); return s.subarray(0, 4 * n); };
    return Object.assign({}, base, {
        sameRatioBatch: P2.refDevice(curve, cv, addon, {}).sameRatioBatch,
        async sectionCheck(_cv, group, tau, nTau, lagrange, top, zeroLast, pairSeed32, ladderSeed32) {
            const G = group == 1 ? curve.G1 : curve.G2, sg = 2 * group * cv.n8q;
            const lem = (p) => { const out = new Uint8Array(sg); G.toRprLEM(out, 0, G.toAffine(p)); return out; };
            tau = Uint8Array.from(tau.subarray(0, nTau * sg));
            const u = await G.batchLEMtoU(tau), s = words(pairSeed32, nTau - 1);
            const r1 = nTau > 1 ? lem(await G.multiExpAffine(tau.slice(0, (nTau - 1) * sg), s)) : new Uint8Array(sg);
            const r2 = nTau > 1 ? lem(await G.multiExpAffine(tau.slice(sg), s)) : new Uint8Array(sg);
            if (!lagrange) return { u, r1, r2, ladder: null };
            const ladder = [];
            for (let p = 0; p <= top; p++) {
                const n = 2 ** p, w = Uint8Array.from(words(ladderSeed32, n)), pts = new Uint8Array(n * sg), cut = p == top && zeroLast;
                pts.set(tau.subarray(0, (cut ? n - 1 : n) * sg));
                if (cut) w.fill(0, 4 * (n - 1));
                const left = await G.multiExpAffine(pts, w);
                let wide = new Uint8Array(32 * n);
                for (let i = 0; i < n; i++) wide.set(w.subarray(4 * i, 4 * i + 4), 32 * i);
                wide = await curve.Fr.batchFromMontgomery(await curve.Fr.fft(await curve.Fr.batchToMontgomery(wide)));
                const right = await G.multiExpAffine(Uint8Array.from(lagrange.subarray((n - 1) * sg, (2 * n - 1) * sg)), wide);
                ladder.push(G.eq(left, right));
            }
            return { u, r1, r2, ladder };
        },
    });
}

module.exports = { ROOT, INDEX, G: P2.G, split: P2.split, join: P2.join, caseFile, capture, afterName, sameLines: P2.sameLines, subtleShim: P2.subtleShim, refDevice };
