// snarkjs_amd/js/fflonk_verify_native.js — batch FFLONK verification on the device from Node (csrc/fflonk_verify.hip through the N-API addon). BN254 only.
//
//   const { VerifyingKey } = require("snarkjs_amd/js/fflonk_verify_native.js");
//   const vk = new VerifyingKey(vkJson, { device: 0 });          // the object zKey.exportVerificationKey writes for an FFLONK key (with X_2 and C0)
//   const ok = await vk.verifyMany(publicSignalsList, proofs);    // boolean[], one per proof, the reference's per-proof verdicts
//
// makeVerifier(snarkjs) is what registerAll(snarkjs, { fused: true, verify: { fflonk: true } }) puts behind snarkjs.fflonk.verify: the reference's
// signature, return value and verdict messages (src/fflonk_verify.js:28-137: "FFLONK VERIFIER STARTED", then an error, or "PROOF VERIFIED SUCCESSFULLY"
// (info) / "Invalid Proof" (warn) followed by "FFLONK VERIFIER FINISHED"). The reference's progress lines (the settings block, "> Computing ...", the
// challenge values) are not reproduced. The reference tests the number of public signals first, so a wrong count is -3 whatever the commitments are.
// Where the reference throws — a wrong count and no logger — this returns false. Calls that arrive while a batch of the same key is on the device join
// the next batch; keys stay resident per vk content until uninstallFused.
"use strict";
const path = require("path");

const BN128 = { id: 0, n8: 32, p: 21888242871839275222246405745257275088696311157297823662689037894645226208583n,
                r: 21888242871839275222246405745257275088548364400416034343698204186575808495617n };
// Fr.w[power] of BN254 is Fr.w[28]^(2^(28 - power)); Fr.w[28] = 5^((r - 1) / 2^28) (ffjavascript: the first non-residue is 5)
const W28 = 19103219067921713944291392827692070036145651957329286315305642004821462161904n;
const MESSAGES = { 1: "PROOF VERIFIED SUCCESSFULLY", 0: "Invalid Proof", "-1": "Public inputs are not valid.", "-2": "Proof commitments are not valid",
                   "-3": "Number of public signals does not match with vk" };
const KEY_CONSTS = ["k1", "k2", "w3", "w4", "w8", "wr"];
const PROOF_POINTS = ["C1", "C2", "W1", "W2"];
const PROOF_EVALS = ["ql", "qr", "qm", "qo", "qc", "s1", "s2", "s3", "a", "b", "c", "z", "zw", "t1w", "t2w"];

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
function rootOfUnity(power) {
    let w = W28;
    for (let i = power; i < 28; i++) w = w * w % BN128.r;
    return w;
}

class VerifyingKey {
    constructor(vk, options) {
        const name = vk.curve || "bn128";
        if (vk.protocol !== "fflonk") throw new Error("not an FFLONK verifying key");
        if (name !== "bn128") throw new Error("FFLONK verification serves bn128 only, not curve " + name + ": the reference has no FFLONK on it");
        const c = this.c = BN128, n8 = c.n8, power = Number(vk.power);
        // the reference reads vk.w in one place and Fr.w[power] in another; one value is used here
        if (vk.w !== undefined && power >= 0 && power <= 28 && mod(big(vk.w), c.r) !== rootOfUnity(power)) throw new Error("vk.w is not Fr.w[power]");
        const A = loadAddon();
        if (options && options.device !== undefined) A.init(options.device);
        this.nPublic = Number(vk.nPublic);
        const c0 = new Uint8Array(3 * n8), x2 = new Uint8Array(6 * n8), consts = new Uint8Array(192);
        g1Bytes(vk.C0, c, c0, 0);
        g2Bytes(vk.X_2, c, x2, 0);
        KEY_CONSTS.forEach((k, i) => putLE(consts, 32 * i, mod(big(vk[k]), c.r), 32));
        this.handle = A.fflonkVkLoad(c.id, c0, x2, consts, power, this.nPublic);
    }
    get recordBytes() { return 12 * this.c.n8 + 480; }
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
            PROOF_POINTS.forEach((k, j) => g1Bytes(pr.polynomials[k], c, recs, i * rec + j * 3 * c.n8));
            PROOF_EVALS.forEach((k, j) => {
                const v = big(pr.evaluations[k]);        // the device reduces modulo r (Fr.fromObject); the host only what does not fit 32 bytes
                putLE(recs, i * rec + 12 * c.n8 + 32 * j, v >= 0n && v < (1n << 256n) ? v : mod(v, c.r), 32);
            });
        }
        return { recs, pubs, nSig, pre };
    }
    async verifyCodes(publicSignalsList, proofs) {
        if (!proofs.length) return [];
        const { recs, pubs, nSig, pre } = this.pack(publicSignalsList, proofs);
        if (nSig !== this.nPublic) {               // the reference tests the count first: -3 whatever the commitments are
            let refused = false;
            try { await loadAddon().fflonkVerifyAsync(this.handle, recs, pubs, nSig, proofs.length); } catch (e) {
                if (!String(e.message).includes(MESSAGES["-3"])) throw e;
                refused = true;
            }
            if (!refused) throw new Error("a wrong number of public signals was not refused");
            return proofs.map(() => -3);
        }
        const out = await loadAddon().fflonkVerifyAsync(this.handle, recs, pubs, nSig, proofs.length);
        const codes = new Int8Array(out.buffer, out.byteOffset, out.length);
        return Array.from(codes, (v, i) => (pre[i] !== null && v !== -2 ? pre[i] : v));
    }
    async verifyMany(publicSignalsList, proofs) {
        return (await this.verifyCodes(publicSignalsList, proofs)).map((v) => v === 1);
    }
    release() {
        if (this.handle) { loadAddon().fflonkVkRelease(this.handle); this.handle = 0; }
    }
}

// snarkjs.fflonk.verify on the device: keys resident per vk content; concurrent calls of one key (and one public-signal count) coalesce into batches
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
                if (b.logger) {
                    if (code === 1) b.logger.info(MESSAGES[1]); else if (code === 0) b.logger.warn(MESSAGES[0]); else b.logger.error(MESSAGES[code]);
                    if (code === 0 || code === 1) b.logger.info("FFLONK VERIFIER FINISHED");
                }
                b.resolve(code === 1);
            });
        }, (err) => batch.forEach((b) => b.reject(err))).then(() => { q.busy = false; pump(e, q); });
    }
    async function verify(vk, publicSignals, proof, logger) {
        stats.calls++;
        const e = entryOf(vk);
        if (logger) logger.info("FFLONK VERIFIER STARTED");
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
