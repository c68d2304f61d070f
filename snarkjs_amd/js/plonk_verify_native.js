// snarkjs_amd/js/plonk_verify_native.js — batch PLONK verification on the device from Node (csrc/plonk_verify.hip through the N-API addon).
//
//   const { VerifyingKey } = require("snarkjs_amd/js/plonk_verify_native.js");
//   const vk = new VerifyingKey(vkJson, { device: 0 });          // the object zKey.exportVerificationKey writes for a PLONK key (with X_2)
//   const ok = await vk.verifyMany(publicSignalsList, proofs);    // boolean[], one per proof, the reference's per-proof verdicts
//
// makeVerifier(snarkjs) is what registerAll(snarkjs, { fused: true, verify: { plonk: true } }) puts behind snarkjs.plonk.verify: the reference's
// signature, return value and logger messages (src/plonk_verify.js:29-123: "PLONK VERIFIER STARTED", then "OK!" (info), "Invalid Proof" (warn) or an
// error). Where the reference throws — a bad commitment and no logger — this returns false. Calls that arrive while a batch of the same key is on the
// device join the next batch; keys stay resident per vk content until uninstallFused.
"use strict";
const path = require("path");

const CURVES = {
    bn128: { id: 0, n8: 32, b: 3n, p: 21888242871839275222246405745257275088696311157297823662689037894645226208583n,
             r: 21888242871839275222246405745257275088548364400416034343698204186575808495617n },
    bls12381: { id: 1, n8: 48, b: 4n, p: 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaabn,
                r: 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001n },
};
const MESSAGES = { 1: "OK!", 0: "Invalid Proof", "-1": "Public inputs are not valid.", "-2": "Proof commitments are not valid.", "-3": "Invalid number of public inputs" };
const KEY_POINTS = ["Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3"];
const PROOF_POINTS = ["A", "B", "C", "Z", "T1", "T2", "T3", "Wxi", "Wxiw"];
const PROOF_EVALS = ["eval_a", "eval_b", "eval_c", "eval_s1", "eval_s2", "eval_zw"];

let addon = null;
function loadAddon() {
    if (!addon) addon = require(path.join(__dirname, "..", "napi", "zkmi_napi.node"));
    return addon;
}
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
// G1.isValid of a point in object form: only used to keep the reference's order (commitments before the signal count) for a call the device refuses as a whole
function onCurve(o, c) {
    const [x, y, z] = [o[0], o[1], o.length > 2 ? o[2] : 1].map((v) => mod(big(v), c.p));
    if (z === 0n) return true;
    const z2 = z * z % c.p;
    return mod(y * y - x * x * x - c.b * z2 * z2 * z2, c.p) === 0n;
}

class VerifyingKey {
    constructor(vk, options) {
        const name = vk.curve || "bn128";
        this.c = CURVES[name];
        if (!this.c) throw new Error("unsupported curve " + name);
        if (vk.protocol !== "plonk") throw new Error("not a PLONK verifying key");
        const A = loadAddon();
        if (options && options.device !== undefined) A.init(options.device);
        const c = this.c, n8 = c.n8;
        this.nPublic = Number(vk.nPublic);
        const g1 = new Uint8Array(24 * n8), x2 = new Uint8Array(6 * n8), k1 = new Uint8Array(32), k2 = new Uint8Array(32);
        KEY_POINTS.forEach((k, i) => g1Bytes(vk[k], c, g1, i * 3 * n8));
        g2Bytes(vk.X_2, c, x2, 0);
        putLE(k1, 0, mod(big(vk.k1), c.r), 32);
        putLE(k2, 0, mod(big(vk.k2), c.r), 32);
        this.handle = A.plonkVkLoad(c.id, g1, x2, k1, k2, Number(vk.power), this.nPublic);
    }
    get recordBytes() { return 27 * this.c.n8 + 192; }
    // packed records + per-proof verdicts decided on the host (a public outside [0, r) may have no 32-byte form: -1, unless a commitment is bad)
    pack(publicSignalsList, proofs) {
        const n = proofs.length, c = this.c, rec = this.recordBytes;
        if (publicSignalsList.length !== n) throw new Error("one publicSignals list per proof");
        const nSig = n ? publicSignalsList[0].length : this.nPublic;
        const recs = new Uint8Array(n * rec), pubs = new Uint8Array(n * nSig * 32), pre = new Array(n).fill(null);
        for (let i = 0; i < n; i++) {
            const sig = publicSignalsList[i], pr = proofs[i];
            if (sig.length !== nSig) throw new Error("every proof of a batch needs the same number of public signals");
            const vals = sig.map(big);
            if (vals.some((v) => v < 0n || v >= c.r)) pre[i] = -1;
            else vals.forEach((v, k) => putLE(pubs, (i * nSig + k) * 32, v, 32));
            PROOF_POINTS.forEach((k, j) => g1Bytes(pr[k], c, recs, i * rec + j * 3 * c.n8));
            PROOF_EVALS.forEach((k, j) => {
                const v = big(pr[k]);                    // the device reduces modulo r (Fr.fromObject); the host only what does not fit 32 bytes
                putLE(recs, i * rec + 27 * c.n8 + 32 * j, v >= 0n && v < (1n << 256n) ? v : mod(v, c.r), 32);
            });
        }
        return { recs, pubs, nSig, pre };
    }
    async verifyCodes(publicSignalsList, proofs) {
        if (!proofs.length) return [];
        const { recs, pubs, nSig, pre } = this.pack(publicSignalsList, proofs);
        if (nSig !== this.nPublic) {
            let refused = false;
            try { await loadAddon().plonkVerifyAsync(this.handle, recs, pubs, nSig, proofs.length); } catch (e) {
                if (!String(e.message).includes(MESSAGES["-3"])) throw e;
                refused = true;
            }
            if (!refused) throw new Error("a wrong number of public signals was not refused");
            return proofs.map((pr) => (PROOF_POINTS.every((k) => onCurve(pr[k], this.c)) ? -3 : -2));
        }
        const out = await loadAddon().plonkVerifyAsync(this.handle, recs, pubs, nSig, proofs.length);
        const codes = new Int8Array(out.buffer, out.byteOffset, out.length);
        return Array.from(codes, (v, i) => (pre[i] !== null && v !== -2 ? pre[i] : v));
    }
    async verifyMany(publicSignalsList, proofs) {
        return (await this.verifyCodes(publicSignalsList, proofs)).map((v) => v === 1);
    }
    release() {
        if (this.handle) { loadAddon().plonkVkRelease(this.handle); this.handle = 0; }
    }
}

// snarkjs.plonk.verify on the device: keys resident per vk content; concurrent calls of one key (and one public-signal count) coalesce into batches
function makeVerifier(snarkjs, options) {
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
                const code = codes[i];
                if (b.logger) { if (code === 1) b.logger.info(MESSAGES[1]); else if (code === 0) b.logger.warn(MESSAGES[0]); else b.logger.error(MESSAGES[code]); }
                b.resolve(code === 1);
            });
        }, (err) => batch.forEach((b) => b.reject(err))).then(() => { q.busy = false; pump(e, q); });
    }
    async function verify(vk, publicSignals, proof, logger) {
        stats.calls++;
        const e = entryOf(vk);
        if (logger) logger.info("PLONK VERIFIER STARTED");
        const nSig = publicSignals.length;
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
}

module.exports = { VerifyingKey, makeVerifier, MESSAGES };
