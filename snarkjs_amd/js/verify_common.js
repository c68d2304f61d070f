// snarkjs_amd/js/verify_common.js — what groth16_verify_native.js, plonk_verify_native.js and fflonk_verify_native.js share: the curves, the addon,
// field-element and point encoding, the public-signal half of a packed batch, and the verifier behind snarkjs.<protocol>.verify (keys resident per vk
// content; calls that arrive while a batch of the same key is on the device join the next batch).
"use strict";
const path = require("path");

const CURVES = {
    bn128: { id: 0, n8: 32, b: 3n, p: 21888242871839275222246405745257275088696311157297823662689037894645226208583n,
             r: 21888242871839275222246405745257275088548364400416034343698204186575808495617n },
    bls12381: { id: 1, n8: 48, b: 4n, p: 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaabn,
                r: 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001n },
};

let addon = null;
function loadAddon() {
    if (!addon) addon = require(path.join(__dirname, "..", "napi", "zkmi_napi.node"));
    return addon;
}
// unstringifyBigInts of one value: decimal or "0x" string, number or bigint
function big(v) {
    if (typeof v === "bigint") return v;
    if (typeof v === "number") return BigInt(v);
    if (typeof v === "string") return BigInt(v);
    throw new TypeError("not a field element: " + v);
}
function putLE(out, off, v, n8) {
    for (let i = 0; i < n8; i++) { out[off + i] = Number(v & 0xffn); v >>= 8n; }
}
function mod(v, p) { const m = v % p; return m < 0n ? m + p : m; }
function g1Bytes(o, c, out, off) {
    const z = o.length > 2 ? o[2] : 1;
    [o[0], o[1], z].forEach((v, k) => putLE(out, off + k * c.n8, mod(big(v), c.p), c.n8));
}
function g2Bytes(o, c, out, off) {
    const z = o.length > 2 ? o[2] : [1, 0];
    [o[0], o[1], z].forEach((e, k) => { putLE(out, off + 2 * k * c.n8, mod(big(e[0]), c.p), c.n8); putLE(out, off + (2 * k + 1) * c.n8, mod(big(e[1]), c.p), c.n8); });
}
// an evaluation: the device reduces modulo r (Fr.fromObject); the host only what does not fit 32 bytes
function frBytes(v, c, out, off) {
    v = big(v);
    putLE(out, off, v >= 0n && v < (1n << 256n) ? v : mod(v, c.r), 32);
}
// G1.isValid of a point in object form
function onCurve(o, c) {
    const [x, y, z] = [o[0], o[1], o.length > 2 ? o[2] : 1].map((v) => mod(big(v), c.p));
    if (z === 0n) return true;
    const z2 = z * z % c.p;
    return mod(y * y - x * x * x - c.b * z2 * z2 * z2, c.p) === 0n;
}

// packed records + per-proof verdicts decided on the host (a public outside [0, r) may have no 32-byte form: -1). record(proof, recs, off) writes a
// proof's rec bytes. Every proof of a batch carries the same number of signals (nSigEmpty for an empty batch); with fewer (Groth16) more signals than
// key.nPublic throw, without it the number is packed as given and a wrong one is left to the device call to refuse.
function pack(key, publicSignalsList, proofs, rec, record, nSigEmpty, fewer) {
    const n = proofs.length, c = key.c;
    if (publicSignalsList.length !== n) throw new Error("one publicSignals list per proof");
    const nSig = n ? publicSignalsList[0].length : nSigEmpty;
    if (fewer && nSig > key.nPublic) throw new Error(nSig + " public signals for a key with nPublic = " + key.nPublic);
    const recs = new Uint8Array(n * rec), pubs = new Uint8Array(n * nSig * 32), pre = new Array(n).fill(null);
    for (let i = 0; i < n; i++) {
        const sig = publicSignalsList[i];
        if (sig.length !== nSig) throw new Error("every proof of a batch needs the same number of public signals");
        const vals = sig.map(big);
        if (vals.some((v) => v < 0n || v >= c.r)) pre[i] = -1;
        else vals.forEach((v, k) => putLE(pubs, (i * nSig + k) * 32, v, 32));
        record(proofs[i], recs, i * rec);
    }
    return { recs, pubs, nSig, pre };
}

// a batch with a wrong number of public signals goes to the device call, which has to refuse it as a whole with message
async function refusedCount(call, message) {
    let refused = false;
    try { await call(); } catch (e) {
        if (!String(e.message).includes(message)) throw e;
        refused = true;
    }
    if (!refused) throw new Error("a wrong number of public signals was not refused");
}

// the aggregated check of a key: "are all of these valid?" by one pairing check for the batch (include/zkmi.h zkmi_*_verify_aggregate).
// aggregateAsync is the addon's *VerifyAggregateAsync, verifyAsync its per-proof call (a wrong number of signals is left to it to refuse, as in
// verifyCodes; null for Groth16, which accepts fewer signals and whose pack() throws on more). options.seed: 32 bytes the maker of the proofs could
// not predict; drawn from the OS unless given.
async function verifyAll(key, aggregateAsync, verifyAsync, countMessage, publicSignalsList, proofs, options) {
    if (!proofs.length) {
        if (publicSignalsList.length) throw new Error("one publicSignals list per proof");
        return true;
    }
    const { recs, pubs, nSig, pre } = key.pack(publicSignalsList, proofs);
    if (verifyAsync && nSig !== key.nPublic) {
        await refusedCount(() => verifyAsync(key.handle, recs, pubs, nSig, proofs.length), countMessage);
        return false;
    }
    if (pre.some((v) => v !== null)) return false;
    let seed = options && options.seed;
    if (seed === undefined || seed === null) seed = require("crypto").randomBytes(32);
    seed = Uint8Array.from(seed);
    if (seed.length !== 32) throw new Error("the seed of an aggregated check is 32 bytes");
    const out = await aggregateAsync(key.handle, recs, pubs, nSig, proofs.length, seed);
    return out[proofs.length] === 1;
}

// hooks: start (the line logged first, or none), log(logger, code) (the verdict's lines), guard(key, nSig) (may throw before a call is queued)
function makeVerifier(VerifyingKey, hooks) {
    return function (snarkjs, options) {
        const keys = new Map();                 // JSON of the vk -> { key, queues: Map(nSig -> { pending, busy }) }
        const stats = { calls: 0, batches: 0 };
        function entryOf(vk) {
            const id = JSON.stringify(vk, (k, v) => (typeof v === "bigint" ? v.toString() : v));
            let e = keys.get(id);
            if (!e) { e = { key: new VerifyingKey(vk, options), queues: new Map() }; keys.set(id, e); }
            return e;
        }
        function pump(e, q) {
            if (q.busy || !q.pending.length) return;
            const batch = q.pending.splice(0, q.pending.length);
            q.busy = true;
            stats.batches++;
            e.key.verifyCodes(batch.map((b) => b.pubs), batch.map((b) => b.proof)).then((codes) => {
                batch.forEach((b, i) => {
                    if (b.logger) hooks.log(b.logger, codes[i]);
                    b.resolve(codes[i] === 1);
                });
            }, (err) => batch.forEach((b) => b.reject(err))).then(() => { q.busy = false; pump(e, q); });
        }
        async function verify(vk, publicSignals, proof, logger) {
            stats.calls++;
            const e = entryOf(vk);
            if (logger && hooks.start) logger.info(hooks.start);
            const nSig = publicSignals.length;
            if (hooks.guard) hooks.guard(e.key, nSig);
            let q = e.queues.get(nSig);
            if (!q) { q = { pending: [], busy: false }; e.queues.set(nSig, q); }
            return new Promise((resolve, reject) => {
                q.pending.push({ pubs: publicSignals, proof, logger, resolve, reject });
                setImmediate(() => pump(e, q));          // let the calls of this turn of the event loop join the batch
            });
        }
        function release() {
            for (const e of keys.values()) { try { e.key.release(); } catch (err) { /* already released */ } }
            keys.clear();
        }
        return { verify, release, stats, keys };
    };
}

module.exports = { CURVES, loadAddon, big, putLE, mod, g1Bytes, g2Bytes, frBytes, onCurve, pack, refusedCount, verifyAll, makeVerifier };
