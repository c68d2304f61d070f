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
const { CURVES, loadAddon, big, putLE, mod, g1Bytes, g2Bytes, frBytes, onCurve, pack, refusedCount, verifyAll, makeVerifier: makeVerifierOf } = require("./verify_common.js");

const MESSAGES = { 1: "OK!", 0: "Invalid Proof", "-1": "Public inputs are not valid.", "-2": "Proof commitments are not valid.", "-3": "Invalid number of public inputs" };
const KEY_POINTS = ["Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3"];
const PROOF_POINTS = ["A", "B", "C", "Z", "T1", "T2", "T3", "Wxi", "Wxiw"];
const PROOF_EVALS = ["eval_a", "eval_b", "eval_c", "eval_s1", "eval_s2", "eval_zw"];

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
        const c = this.c;
        return pack(this, publicSignalsList, proofs, this.recordBytes, (pr, recs, off) => {
            PROOF_POINTS.forEach((k, j) => g1Bytes(pr[k], c, recs, off + j * 3 * c.n8));
            PROOF_EVALS.forEach((k, j) => frBytes(pr[k], c, recs, off + 27 * c.n8 + 32 * j));
        }, this.nPublic, false);
    }
    async verifyCodes(publicSignalsList, proofs) {
        if (!proofs.length) return [];
        const { recs, pubs, nSig, pre } = this.pack(publicSignalsList, proofs);
        if (nSig !== this.nPublic) {
            await refusedCount(() => loadAddon().plonkVerifyAsync(this.handle, recs, pubs, nSig, proofs.length), MESSAGES["-3"]);
            return proofs.map((pr) => (PROOF_POINTS.every((k) => onCurve(pr[k], this.c)) ? -3 : -2));
        }
        const out = await loadAddon().plonkVerifyAsync(this.handle, recs, pubs, nSig, proofs.length);
        const codes = new Int8Array(out.buffer, out.byteOffset, out.length);
        return Array.from(codes, (v, i) => (pre[i] !== null && v !== -2 ? pre[i] : v));
    }
    async verifyMany(publicSignalsList, proofs) {
        return (await this.verifyCodes(publicSignalsList, proofs)).map((v) => v === 1);
    }
    // are all of these valid? One pairing check for the whole batch; equals verifyMany(...).every(Boolean) except with probability about 2^-127 over
    // the seed ({ seed }: 32 bytes, drawn from the OS unless given)
    async verifyAll(publicSignalsList, proofs, options) {
        const A = loadAddon();
        return verifyAll(this, A.plonkVerifyAggregateAsync, A.plonkVerifyAsync, MESSAGES["-3"], publicSignalsList, proofs, options);
    }
    release() {
        if (this.handle) { loadAddon().plonkVkRelease(this.handle); this.handle = 0; }
    }
}

// snarkjs.plonk.verify on the device: keys resident per vk content; concurrent calls of one key (and one public-signal count) coalesce into batches
const makeVerifier = makeVerifierOf(VerifyingKey, {
    start: "PLONK VERIFIER STARTED",
    log(logger, code) {
        if (code === 1) logger.info(MESSAGES[1]); else if (code === 0) logger.warn(MESSAGES[0]); else logger.error(MESSAGES[code]);
    },
});

module.exports = { VerifyingKey, makeVerifier, MESSAGES };
