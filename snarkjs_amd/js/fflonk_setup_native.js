// snarkjs_amd/js/fflonk_setup_native.js — snarkjs.fflonk.setup (src/fflonk_setup.js) through the addon's fflonkSetupLower and fflonkSetup (include/zkmi.h:
// zkmi_fflonk_setup_lower, zkmi_fflonk_setup): setup(r1cs, ptau) -> the key's bytes, byte for byte the reference's, on BN254. The twin of
// snarkjs_amd/fflonk_setup.py. Sources are a Uint8Array with the file's bytes, a path or a fastfile descriptor; sections are read by offset (readerOf /
// sectionTable of groth16_native.js), a large ptau is never loaded whole. The library lowers the constraints on the host (sections 3 - 6) and computes
// sections 7 - 15, section 17 and the C0 commitment on the device; this file writes sections 1, 2 and 16 and puts the 17 sections in the reference's order.
"use strict";
const path = require("path");
const { readerOf, sectionTable } = require("./groth16_native.js");
const { SetupRefusal } = require("./groth16_setup_native.js");
const { bigToLe, u32, log2, readPtauHeader, readR1csHeader, zkeyWriter } = require("./gate_setup_io.js");

const Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583n;
const R = 21888242871839275222246405745257275088548364400416034343698204186575808495617n;
const N8Q = 32, SG1 = 64, SG2 = 128;

function powMod(b, e) { let r = 1n; b %= R; while (e > 0n) { if (e & 1n) r = r * b % R; b = b * b % R; e >>= 1n; } return r; }
const mont = (v) => bigToLe((v << 256n) % R, 32);
// Fr.w[i] of ffjavascript on BN254
const frRoot = (i) => powMod(powMod(5n, (R - 1n) >> 28n), 1n << BigInt(28 - i));

// whether the ceremony is on bn128: every other curve stays with the reference (register.js)
function isBn128(ptauSrc) {
    const pt = readerOf(ptauSrc);
    try { return readPtauHeader(pt, sectionTable(pt, "ptau")).q === Q; } catch (e) { return false; } finally { pt.close(); }
}

function setup(r1csSrc, ptauSrc, options) {
    options = options || {};
    const addon = options.addon || require(path.join(__dirname, "..", "napi", "zkmi_napi.node"));
    const logger = options.logger;
    const pt = readerOf(ptauSrc);
    let r1;
    try {
        const sp = sectionTable(pt, "ptau");
        if (!sp[12]) throw new SetupRefusal("Powers of Tau is not well prepared. Section 12 missing.");
        const { q } = readPtauHeader(pt, sp);
        if (q !== Q && q !== 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaabn) throw new Error(`Curve not supported: ${q}`);
        const ptauR = q === Q ? R : 52435875175126190479447740508185965837690552500527637822603658699938581184513n;
        r1 = readerOf(r1csSrc);
        const sr = sectionTable(r1, "r1cs");
        const { prime, nVars, nOutputs, nPubInputs, nConstraints } = readR1csHeader(r1, sr);
        const nPublic = nOutputs + nPubInputs;
        if (prime !== ptauR) throw new SetupRefusal("r1cs curve does not match powers of tau ceremony curve");
        if (q !== Q) throw new SetupRefusal("fflonk.setup is not supported on BLS12-381: the reference writes BN254's w3 and wr into the key, so no proof under it verifies");
        if (logger) logger.info("> Processing FFlonk constraints");
        const low = addon.fflonkSetupLower(0, nConstraints, nVars, nPublic, r1.read(sr[2][0].pos, sr[2][0].len));
        const cirPower = Math.max(3, log2(low.nConstraints + 1) + 1), domainSize = 2 ** cirPower;
        if (domainSize !== low.domainSize) throw new Error("fflonk.setup: the library's domainSize differs from the reference's formula");
        if (sp[2][0].len < (domainSize * 9 + 18) * SG1) throw new SetupRefusal("Powers of Tau is not big enough for this circuit size. Section 2 too small.");
        if (sp[3][0].len < SG2) throw new SetupRefusal("Powers of Tau is not well prepared. Section 3 too small.");
        if (logger) { logger.info(`  Constraints:   ${low.nConstraints}`); logger.info(`  Additions:     ${low.nAdditions}`); }
        const sec16 = pt.read(sp[2][0].pos, (domainSize * 9 + 18) * SG1);
        const dev = addon.fflonkSetup(0, nPublic, low.nConstraints, domainSize, low.selectors, low.pred, sec16.subarray(0, 8 * domainSize * SG1));
        // computeK1K2 (:513-532) calls Fr.add without assigning its result: k1 = 2 and k2 = 3, or it never returns
        // computeW3 (:534-542): its "order(r - 1)" constant is (r - 1) / 6
        const w3 = powMod(31624n, 3648040478639879203707734290876212514758060733402672390616367364429301415936n / 3n), wr = powMod(467799165886069610036046866799264026481344299079011762026774533774345988080n, 1n << BigInt(28 - cirPower));
        const sec2 = Buffer.concat([u32(N8Q), bigToLe(Q, N8Q), u32(32), bigToLe(R, 32), u32(low.plonkNVars), u32(nPublic), u32(domainSize), u32(low.nAdditions),
                                    u32(low.nConstraints), mont(2n), mont(3n), mont(w3), mont(frRoot(2)), mont(frRoot(3)), mont(wr), pt.read(sp[3][0].pos + SG2, SG2), dev.commitment]);
        const key = zkeyWriter(17), sec = key.sec;
        const rec = 5 * domainSize * 32;
        sec(1, u32(10));
        sec(3, low.additions); sec(4, low.mapA); sec(5, low.mapB); sec(6, low.mapC);
        for (let i = 0; i < 5; i++) sec(7 + i, dev.q[i]);
        for (let i = 0; i < 3; i++) sec(12 + i, dev.sigma.subarray(i * rec, (i + 1) * rec));
        sec(15, dev.lagrange); sec(16, sec16); sec(17, dev.c0);
        sec(2, sec2);
        return key.bytes();
    } finally {
        pt.close();
        if (r1) r1.close();
    }
}

module.exports = { setup, isBn128, SetupRefusal };
