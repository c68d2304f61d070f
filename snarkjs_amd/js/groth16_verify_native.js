// snarkjs_amd/js/groth16_verify_native.js — batch Groth16 verification on the device from Node (csrc/groth16_verify.hip through the N-API addon).
//
//   const { VerifyingKey } = require("snarkjs_amd/js/groth16_verify_native.js");
//   const vk = new VerifyingKey(vkJson, { device: 0 });          // the object zKey.exportVerificationKey writes
//   const ok = await vk.verifyMany(publicSignalsList, proofs);    // boolean[], one per proof, the reference's per-proof verdicts
//
// makeVerifier(snarkjs) is what registerAll(snarkjs, { fused: true, verify: true }) puts behind snarkjs.groth16.verify: the reference's signature,
// return value and logger messages (src/groth16_verify.js:26-87); calls that arrive while a batch of the same key is on the device join the next batch;
// keys stay resident per vk content until uninstallFused.
"use strict";
const path = require("path");

const CURVES = {
    bn128: { id: 0, n8: 32, p: 21888242871839275222246405745257275088696311157297823662689037894645226208583n,
             r: 21888242871839275222246405745257275088548364400416034343698204186575808495617n },
    bls12381: { id: 1, n8: 48, p: 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaabn,
                r: 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001n },
};
const MESSAGES = { 1: "OK!", 0: "Invalid proof", "-1": "Public inputs are not valid.", "-2": "Proof commitments are not valid." };

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

class VerifyingKey {
    constructor(vk, options) {
        const name = vk.curve || "bn128";
        this.c = CURVES[name];
        if (!this.c) throw new Error("unsupported curve " + name);
        const A = loadAddon();
        if (options && options.device !== undefined) A.init(options.device);
        const c = this.c, n8 = c.n8;
        this.nPublic = vk.IC.length - 1;
        const al = new Uint8Array(3 * n8), be = new Uint8Array(6 * n8), ga = new Uint8Array(6 * n8), de = new Uint8Array(6 * n8);
        const ic = new Uint8Array(vk.IC.length * 3 * n8);
        g1Bytes(vk.vk_alpha_1, c, al, 0); g2Bytes(vk.vk_beta_2, c, be, 0); g2Bytes(vk.vk_gamma_2, c, ga, 0); g2Bytes(vk.vk_delta_2, c, de, 0);
        vk.IC.forEach((p, i) => g1Bytes(p, c, ic, i * 3 * n8));
        this.handle = A.groth16VkLoad(c.id, al, be, ga, de, ic, this.nPublic);
    }
    // packed records + per-proof verdicts decided on the host (a public outside [0, r) has no 32-byte form: -1, as publicInputsAreValid)
    pack(publicSignalsList, proofs) {
        const n = proofs.length, c = this.c, rec = 12 * c.n8;
        if (publicSignalsList.length !== n) throw new Error("one publicSignals list per proof");
        const nSig = n ? publicSignalsList[0].length : 0;
        if (nSig > this.nPublic) throw new Error(nSig + " public signals for a key with nPublic = " + this.nPublic);
        const recs = new Uint8Array(n * rec), pubs = new Uint8Array(n * nSig * 32), pre = new Array(n).fill(null);
        for (let i = 0; i < n; i++) {
            const sig = publicSignalsList[i], pr = proofs[i];
            if (sig.length !== nSig) throw new Error("every proof of a batch needs the same number of public signals");
            const vals = sig.map(big);
            if (vals.some((v) => v < 0n || v >= c.r)) pre[i] = -1;
            else vals.forEach((v, k) => putLE(pubs, (i * nSig + k) * 32, v, 32));
            g1Bytes(pr.pi_a, c, recs, i * rec);
            g2Bytes(pr.pi_b, c, recs, i * rec + 3 * c.n8);
            g1Bytes(pr.pi_c, c, recs, i * rec + 9 * c.n8);
        }
        return { recs, pubs, nSig, pre };
    }
    async verifyCodes(publicSignalsList, proofs) {
        if (!proofs.length) return [];
        const { recs, pubs, nSig, pre } = this.pack(publicSignalsList, proofs);
        const out = await loadAddon().groth16VerifyAsync(this.handle, recs, pubs, nSig, proofs.length);
        const codes = new Int8Array(out.buffer, out.byteOffset, out.length);
        return Array.from(codes, (v, i) => (pre[i] !== null ? pre[i] : v));
    }
    async verifyMany(publicSignalsList, proofs) {
        return (await this.verifyCodes(publicSignalsList, proofs)).map((v) => v === 1);
    }
    release() {
        if (this.handle) { loadAddon().groth16VkRelease(this.handle); this.handle = 0; }
    }
}

// snarkjs.groth16.verify on the device: keys resident per vk content; concurrent calls of one key (and one public-signal count) coalesce into batches
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
                if (b.logger) { if (code === 1) b.logger.info(MESSAGES[1]); else b.logger.error(MESSAGES[code]); }
                b.resolve(code === 1);
            });
        }, (err) => batch.forEach((b) => b.reject(err))).then(() => { q.busy = false; pump(e, q); });
    }
    async function verify(vk, publicSignals, proof, logger) {
        stats.calls++;
        const e = entryOf(vk);
        const nSig = publicSignals.length;
        if (nSig > e.key.nPublic) throw new TypeError("more public signals than the key's IC points");      // the reference fails reading IC[i + 1]
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
