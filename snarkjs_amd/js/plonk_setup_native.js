// snarkjs_amd/js/plonk_setup_native.js — snarkjs.plonk.setup (src/plonk_setup.js) through the addon's plonkSetupLower and plonkSetup (include/zkmi.h:
// zkmi_plonk_setup_lower, zkmi_plonk_setup): setup(r1cs, ptau) -> the key's bytes, byte for byte the reference's. The twin of snarkjs_amd/plonk_setup.py.
// Sources are a Uint8Array with the file's bytes, a path or a fastfile descriptor; sections are read by offset (readerOf / sectionTable of
// groth16_native.js), a large ptau is never loaded whole. The library lowers the constraints on the host (sections 3 - 6) and computes sections 7 - 13
// and the eight commitments on the device; this file writes sections 1, 2 and 14 and puts the 14 sections in the reference's order.
"use strict";
const path = require("path");
const { readerOf, sectionTable } = require("./groth16_native.js");
const { SetupRefusal } = require("./groth16_setup_native.js");
const { bigToLe, u32, log2, readPtauHeader, readR1csHeader, zkeyWriter } = require("./gate_setup_io.js");

const CURVES = [
    { name: "bn128", id: 0, n8q: 32,
      q: 21888242871839275222246405745257275088696311157297823662689037894645226208583n,
      r: 21888242871839275222246405745257275088548364400416034343698204186575808495617n },
    { name: "bls12381", id: 1, n8q: 48,
      q: 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaabn,
      r: 52435875175126190479447740508185965837690552500527637822603658699938581184513n },
];

function setup(r1csSrc, ptauSrc, options) {
    options = options || {};
    const addon = options.addon || require(path.join(__dirname, "..", "napi", "zkmi_napi.node"));
    const logger = options.logger;
    const pt = readerOf(ptauSrc);
    let r1;
    try {
        const sp = sectionTable(pt, "ptau");
        const { q, power } = readPtauHeader(pt, sp);
        const cv = CURVES.find((c) => c.q === q);
        if (!cv) throw new Error(`Curve not supported: ${q}`);
        r1 = readerOf(r1csSrc);
        const sr = sectionTable(r1, "r1cs");
        const { n8: rn8, prime, nVars, nOutputs, nPubInputs, nConstraints } = readR1csHeader(r1, sr);
        const nPublic = nOutputs + nPubInputs, sG1 = 2 * cv.n8q, sG2 = 4 * cv.n8q;
        if (logger) logger.info("Reading r1cs");
        // the reference lowers the constraints before it compares the curves (:62-72); a field of another width cannot be lowered at all
        if (rn8 !== 32) throw new SetupRefusal("r1cs curve does not match powers of tau ceremony curve");
        const low = addon.plonkSetupLower(cv.id, nConstraints, nVars, nPublic, r1.read(sr[2][0].pos, sr[2][0].len));
        if (prime !== cv.r) throw new SetupRefusal("r1cs curve does not match powers of tau ceremony curve");
        const cirPower = Math.max(3, log2(low.nConstraints - 1) + 1), domainSize = 2 ** cirPower;
        if (domainSize !== low.domainSize) throw new Error("plonk.setup: the library's domainSize differs from the reference's formula");
        if (logger) logger.info("Plonk constraints: " + low.nConstraints);
        if (cirPower > power) throw new SetupRefusal(`circuit too big for this power of tau ceremony. ${low.nConstraints} > 2**${power}`);
        if (!sp[12]) throw new SetupRefusal("Powers of tau is not prepared.");
        const dev = addon.plonkSetup(cv.id, nPublic, low.nConstraints, domainSize, low.selectors, low.pred, pt.read(sp[12][0].pos + (domainSize - 1) * sG1, domainSize * sG1));
        // getK1K2 (:484-504) calls Fr.add without assigning its result: k1 = 2 and k2 = 3, or it never returns
        const mont = (v) => bigToLe((v << 256n) % cv.r, 32);
        const sec2 = Buffer.concat([u32(cv.n8q), bigToLe(cv.q, cv.n8q), u32(32), bigToLe(cv.r, 32), u32(low.plonkNVars), u32(nPublic), u32(domainSize), u32(low.nAdditions),
                                    u32(low.nConstraints), mont(2n), mont(3n), dev.commitments, pt.read(sp[3][0].pos + sG2, sG2)]);
        const key = zkeyWriter(14), sec = key.sec;
        sec(3, low.additions); sec(4, low.mapA); sec(5, low.mapB); sec(6, low.mapC);
        for (let i = 0; i < 5; i++) sec(7 + i, dev.q[i]);
        sec(12, dev.sigma); sec(13, dev.lagrange);
        sec(14, pt.read(sp[2][0].pos, (domainSize + 6) * sG1));
        sec(1, u32(2)); sec(2, sec2);
        return key.bytes();
    } finally {
        pt.close();
        if (r1) r1.close();
    }
}

module.exports = { setup, SetupRefusal };
