// snarkjs_amd/js/groth16_verify_native.js — batch Groth16 verification on the device from Node (csrc/groth16_verify.hip through the N-API addon).
//
//   const { VerifyingKey } = require("snarkjs_amd/js/groth16_verify_native.js");
//   const vk = new VerifyingKey(vkJson, { device: 0 });          // the object zKey.exportVerificationKey writes
//   const ok = await vk.verifyMany(publicSignalsList, proofs);    // boolean[], one per proof, the reference's per-proof verdicts
//   const all = await vk.verifyAll(publicSignalsList, proofs);    // boolean: are all of them valid? One final exponentiation for the batch
//
// makeVerifier(snarkjs) is what registerAll(snarkjs, { fused: true, verify: true }) puts behind snarkjs.groth16.verify: the reference's signature,
// return value and logger messages (src/groth16_verify.js:26-87); calls that arrive while a batch of the same key is on the device join the next batch;
// keys stay resident per vk content until uninstallFused.
"use strict";
const { CURVES, loadAddon, g1Bytes, g2Bytes, pack, verifyAll, makeVerifier: makeVerifierOf } = require("./verify_common.js");

const MESSAGES = { 1: "OK!", 0: "Invalid proof", "-1": "Public inputs are not valid.", "-2": "Proof commitments are not valid." };

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
        const c = this.c;
        return pack(this, publicSignalsList, proofs, 12 * c.n8, (pr, recs, off) => {
            g1Bytes(pr.pi_a, c, recs, off);
            g2Bytes(pr.pi_b, c, recs, off + 3 * c.n8);
            g1Bytes(pr.pi_c, c, recs, off + 9 * c.n8);
        }, 0, true);
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
    // are all of these valid? One Miller loop per proof and ONE final exponentiation for the batch; equals verifyMany(...).every(Boolean) except with
    // probability about 2^-127 over the seed ({ seed }: 32 bytes, drawn from the OS unless given)
    async verifyAll(publicSignalsList, proofs, options) {
        return verifyAll(this, loadAddon().groth16VerifyAggregateAsync, null, null, publicSignalsList, proofs, options);
    }
    release() {
        if (this.handle) { loadAddon().groth16VkRelease(this.handle); this.handle = 0; }
    }
}

// snarkjs.groth16.verify on the device: keys resident per vk content; concurrent calls of one key (and one public-signal count) coalesce into batches
const makeVerifier = makeVerifierOf(VerifyingKey, {
    log(logger, code) { if (code === 1) logger.info(MESSAGES[1]); else logger.error(MESSAGES[code]); },
    guard(key, nSig) { if (nSig > key.nPublic) throw new TypeError("more public signals than the key's IC points"); },      // the reference fails reading IC[i + 1]
});

module.exports = { VerifyingKey, makeVerifier, MESSAGES };
