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
const { CURVES, loadAddon, big, putLE, mod, g1Bytes, g2Bytes, frBytes, pack, refusedCount, verifyAll, makeVerifier: makeVerifierOf } = require("./verify_common.js");

const BN128 = CURVES.bn128;
// Fr.w[power] of BN254 is Fr.w[28]^(2^(28 - power)); Fr.w[28] = 5^((r - 1) / 2^28) (ffjavascript: the first non-residue is 5)
const W28 = 19103219067921713944291392827692070036145651957329286315305642004821462161904n;
const MESSAGES = { 1: "PROOF VERIFIED SUCCESSFULLY", 0: "Invalid Proof", "-1": "Public inputs are not valid.", "-2": "Proof commitments are not valid",
                   "-3": "Number of public signals does not match with vk" };
const KEY_CONSTS = ["k1", "k2", "w3", "w4", "w8", "wr"];
const PROOF_POINTS = ["C1", "C2", "W1", "W2"];
const PROOF_EVALS = ["ql", "qr", "qm", "qo", "qc", "s1", "s2", "s3", "a", "b", "c", "z", "zw", "t1w", "t2w"];

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
        const c = this.c;
        return pack(this, publicSignalsList, proofs, this.recordBytes, (pr, recs, off) => {
            PROOF_POINTS.forEach((k, j) => g1Bytes(pr.polynomials[k], c, recs, off + j * 3 * c.n8));
            PROOF_EVALS.forEach((k, j) => frBytes(pr.evaluations[k], c, recs, off + 12 * c.n8 + 32 * j));
        }, this.nPublic, false);
    }
    async verifyCodes(publicSignalsList, proofs) {
        if (!proofs.length) return [];
        const { recs, pubs, nSig, pre } = this.pack(publicSignalsList, proofs);
        if (nSig !== this.nPublic) {               // the reference tests the count first: -3 whatever the commitments are
            await refusedCount(() => loadAddon().fflonkVerifyAsync(this.handle, recs, pubs, nSig, proofs.length), MESSAGES["-3"]);
            return proofs.map(() => -3);
        }
        const out = await loadAddon().fflonkVerifyAsync(this.handle, recs, pubs, nSig, proofs.length);
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
        return verifyAll(this, A.fflonkVerifyAggregateAsync, A.fflonkVerifyAsync, MESSAGES["-3"], publicSignalsList, proofs, options);
    }
    release() {
        if (this.handle) { loadAddon().fflonkVkRelease(this.handle); this.handle = 0; }
    }
}

// snarkjs.fflonk.verify on the device: keys resident per vk content; concurrent calls of one key (and one public-signal count) coalesce into batches
const makeVerifier = makeVerifierOf(VerifyingKey, {
    start: "FFLONK VERIFIER STARTED",
    log(logger, code) {
        if (code === 1) logger.info(MESSAGES[1]); else if (code === 0) logger.warn(MESSAGES[0]); else logger.error(MESSAGES[code]);
        if (code === 0 || code === 1) logger.info("FFLONK VERIFIER FINISHED");
    },
});

module.exports = { VerifyingKey, makeVerifier, MESSAGES };
