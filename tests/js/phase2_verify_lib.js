// tests/js/phase2_verify_lib.js — shared by phase2_verify_gpu.js and phase2_verify_cpu.js: golden keys taken apart and put together again, the lines a
// verifyFromInit call sends to console.log and to its logger, and the three device calls of js/groth16_phase2_verify_native.js restated on the reference's
// own curve object (its pairingEq, multiExpAffine, batchApplyKey and fft) with the scalars of the library's sequential generator.
"use strict";
const fs = require("fs"), path = require("path");
const ROOT = path.join(__dirname, "..", "..");
const phase2N = require(path.join(ROOT, "snarkjs_amd", "js", "groth16_phase2_native.js"));
const G = (f) => new Uint8Array(fs.readFileSync(path.join(ROOT, "tests", "golden", f)));

function split(raw) {                                    // [[type, body]] in file order
    const dv = new DataView(raw.buffer, raw.byteOffset, raw.byteLength), out = [];
    let off = 12;
    for (let i = 0, n = dv.getUint32(8, true); i < n; i++) {
        const t = dv.getUint32(off, true), len = Number(dv.getBigUint64(off + 4, true));
        out.push([t, raw.subarray(off + 12, off + 12 + len)]);
        off += 12 + len;
    }
    return out;
}
function join(raw, secs) {
    const parts = [Buffer.from(raw.subarray(0, 8)), Buffer.alloc(4)];
    parts[1].writeUInt32LE(secs.length);
    for (const [t, b] of secs) { const h = Buffer.alloc(12); h.writeUInt32LE(t); h.writeBigUInt64LE(BigInt(b.length), 4); parts.push(h, Buffer.from(b)); }
    return new Uint8Array(Buffer.concat(parts));
}
const withSection = (raw, typ, fn) => join(raw, split(raw).map(([t, b]) => [t, t == typ ? fn(b) : b]));
const sectionOf = (raw, typ) => split(raw).find(([t]) => t == typ)[1];
// the section with the first two distinct points that satisfy pick swapped
function swapPoints(body, size, pick) {
    const out = Uint8Array.from(body), pt = (k) => body.subarray(k * size, (k + 1) * size), n = body.length / size;
    const eq = (a, b) => Buffer.compare(Buffer.from(a), Buffer.from(b)) === 0;
    let i = 0;
    while (!pick(pt(i))) i++;
    let j = i + 1;
    while (!pick(pt(j)) || eq(pt(i), pt(j))) { j++; if (j >= n) throw new Error("no second point"); }
    out.set(pt(j), i * size); out.set(pt(i), j * size);
    return out;
}
function withContribution(cv, raw, i, edit) {
    return withSection(raw, 10, (sec) => { const mpc = phase2N.parseMpcParams(Uint8Array.from(sec), cv); edit(mpc.contributions[i]); return phase2N.serialiseMpcParams(mpc); });
}

// run f(logger) with console.log captured: { result | error, lines: [[level, text]] }
async function capture(f) {
    const lines = [], logger = {};
    for (const level of ["error", "info", "debug", "warn"]) logger[level] = (m) => lines.push([level, String(m)]);
    const saved = console.log;
    console.log = (...a) => lines.push(["log", a.join(" ")]);
    try { return { result: await f(logger), lines }; } catch (e) { return { error: e.message, lines }; } finally { console.log = saved; }
}
// the reference's browser build hashes a beacon through crypto.subtle.digest, which the shim's crypto object lacks (call after requiring oracle/ref_shim.js)
function subtleShim() {
    const nodeCrypto = require("crypto");
    globalThis.crypto.subtle = { digest: async (alg, ab) => { const d = nodeCrypto.createHash("sha256").update(Buffer.from(ab)).digest(); return d.buffer.slice(d.byteOffset, d.byteOffset + d.byteLength); } };
}
const sameLines =(a, b) => JSON.stringify(a) === JSON.stringify(b);

// the three calls on the reference's curve (ffjavascript's WASM): what the kernels are to compute, by the reference's own arithmetic
function refDevice(curve, cv, addon, base) {
    const G1 = curve.G1, G2 = curve.G2, Fr = curve.Fr, s1 = 2 * cv.n8q;
    const seedWords = (b32) => { const w = new Uint32Array(8), b = Buffer.from(b32.buffer, b32.byteOffset, 32); for (let i = 0; i < 8; i++) w[i] = b.readUInt32BE(4 * i); return w; };
    const lem = (p) => { const out = new Uint8Array(s1); G1.toRprLEM(out, 0, G1.toAffine(p)); return out; };
    return Object.assign({}, base, {
        async sameRatioBatch(_cv, checks) {
            const out = [];
            for (const c of checks) {
                const a = G1.fromRprLEM(Uint8Array.from(c[0]), 0), ax = G1.fromRprLEM(Uint8Array.from(c[1]), 0), b = G2.fromRprLEM(Uint8Array.from(c[2]), 0), bx = G2.fromRprLEM(Uint8Array.from(c[3]), 0);
                if (G1.isZero(a) || G1.isZero(ax) || G2.isZero(b) || G2.isZero(bx)) { out.push(false); continue; }
                out.push((await curve.pairingEq(a, bx, G1.neg(ax), b)) === true);
            }
            return out;
        },
        async sectionRatio(_cv, a, b, n, seed32) {
            const s = new Uint8Array(4 * n);
            addon.call("zkmi_chacha_struct_words_host", seedWords(seed32), 0, s, n);
            return [lem(await G1.multiExpAffine(Uint8Array.from(a), s)), lem(await G1.multiExpAffine(Uint8Array.from(b), s))];
        },
        async hRatio(_cv, tau, h, power, seed32) {
            const dom = 2 ** power, raw = new Uint8Array(32 * dom);
            addon.call("zkmi_chacha_fr_host", cv.id, seedWords(seed32), raw, dom - 1, null);
            const e = await Fr.batchFromMontgomery(raw), es = e.slice(0, 32 * (dom - 1));
            const hi = await G1.multiExpAffine(Uint8Array.from(tau.subarray(dom * s1, (2 * dom - 1) * s1)), es), lo = await G1.multiExpAffine(Uint8Array.from(tau.subarray(0, (dom - 1) * s1)), es);
            let t = await Fr.batchApplyKey(raw, Fr.neg(Fr.e(2)), Fr.w[power + 1]);
            t = await Fr.batchFromMontgomery(await Fr.fft(t));
            return [lem(G1.sub(hi, lo)), lem(await G1.multiExpAffine(Uint8Array.from(h), t))];
        },
    });
}

module.exports = { ROOT, G, split, join, withSection, sectionOf, swapPoints, withContribution, capture, sameLines, refDevice, subtleShim };
