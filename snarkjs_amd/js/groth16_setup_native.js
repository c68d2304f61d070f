// snarkjs_amd/js/groth16_setup_native.js — snarkjs.zKey.newZKey (src/zkey_new.js) through the addon's groth16Setup (include/zkmi.h:
// zkmi_groth16_setup): newZKey(r1cs, ptau) -> { zkey, csHash }, byte for byte the reference's key. The twin of snarkjs_amd/groth16_setup.py.
// Sources are a Uint8Array with the file's bytes, a path or a fastfile descriptor; sections are read by offset (readerOf / sectionTable of
// groth16_native.js), a large ptau is never loaded whole. The device computes sections 3 - 8 and the H points of the circuit hash; this file
// writes sections 1, 2, 9, 10 and feeds the hash (Blake2b-512) in the reference's order.
"use strict";
const crypto = require("crypto"), path = require("path");
const { readerOf, sectionTable } = require("./groth16_native.js");

const CURVES = [
    { name: "bn128", id: 0, n8q: 32, s: 28,
      q: 21888242871839275222246405745257275088696311157297823662689037894645226208583n,
      r: 21888242871839275222246405745257275088548364400416034343698204186575808495617n,
      g1: [1n, 2n],
      g2: [10857046999023057135944570762232829481370756359578518086990519993285655852781n, 11559732032986387107991004021392285783925812861821192530917403151452391805634n,
           8495653923123431417604973247489272438418190587263600148770280649306958101930n, 4082367875863433681332203403145435568316851327593401208105741076214120093531n] },
    { name: "bls12381", id: 1, n8q: 48, s: 32,
      q: 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaabn,
      r: 52435875175126190479447740508185965837690552500527637822603658699938581184513n,
      g1: [0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bbn,
           0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1n],
      g2: [0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8n,
           0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7en,
           0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801n,
           0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79ben] },
];
const HASH_CHUNK = 1 << 14;            // CHUNK_SIZE of hashHPoints (src/zkey_new.js:505)

// what the reference refuses: it logs `message` and returns -1 (throws when `throws`); handOver: the one call left to the reference itself
class SetupRefusal extends Error {
    constructor(message, flags) { super(message); Object.assign(this, flags || {}); }
}

function leToBig(b) { let v = 0n; for (let i = b.length - 1; i >= 0; i--) v = (v << 8n) | BigInt(b[i]); return v; }
function bigToLe(v, n) { const o = new Uint8Array(n); for (let i = 0; i < n; i++) { o[i] = Number(v & 0xffn); v >>= 8n; } return o; }
function bigToBe(v, n) { return bigToLe(v, n).reverse(); }
function modpow(b, e, m) { let r = 1n; b %= m; while (e > 0n) { if (e & 1n) r = r * b % m; b = b * b % m; e >>= 1n; } return r; }
function u32(v, le) { const b = Buffer.alloc(4); if (le) b.writeUInt32LE(v >>> 0); else b.writeUInt32BE(v >>> 0); return b; }
function log2(v) { return v > 0 ? 31 - Math.clz32(v) : 0; }

// The (offset, count) ranges hashHPoints feeds to the circuit hash (:504-514): n = min(domainSize - 1, CHUNK_SIZE) for EVERY chunk, so from
// domainSize = 2^15 on the last chunk ends at point domainSize - 1, one past the domainSize - 1 points announced.
function hashHChunks(domainSize) {
    const out = [], n = Math.min(domainSize - 1, HASH_CHUNK);
    for (let i = 0; i < domainSize - 1; i += HASH_CHUNK) out.push([i, n]);
    return out;
}
function hashedHPoints(domainSize) { const c = hashHChunks(domainSize); return c.length ? c[c.length - 1][0] + c[c.length - 1][1] : 0; }

// batchLEMtoU of a few header points on the host: big-endian normal form, an Fq2 coordinate as c1 || c0
function lemToUHost(cv, buf, group) {
    const n8 = cv.n8q, rinv = modpow(1n << BigInt(8 * n8), cv.q - 2n, cv.q), el = [];
    for (let o = 0; o < buf.length; o += n8) el.push(bigToBe(leToBig(buf.subarray(o, o + n8)) * rinv % cv.q, n8));
    return Buffer.concat(group == 2 ? el.map((_, i) => el[i ^ 1]) : el);
}
function generatorsLem(cv) {
    const m = (v) => bigToLe((v << BigInt(8 * cv.n8q)) % cv.q, cv.n8q);
    return { g1: Buffer.concat(cv.g1.map(m)), g2: Buffer.concat(cv.g2.map(m)) };
}

function newZKey(r1csSrc, ptauSrc, options) {
    options = options || {};
    const addon = options.addon || require(path.join(__dirname, "..", "napi", "zkmi_napi.node"));
    const pt = readerOf(ptauSrc);
    let r1;
    try {
        const sp = sectionTable(pt, "ptau");
        const h = pt.read(sp[1][0].pos, sp[1][0].len), hv = new DataView(h.buffer, h.byteOffset, h.byteLength);
        const n8 = hv.getUint32(0, true), q = leToBig(h.subarray(4, 4 + n8));
        const cv = CURVES.find((c) => c.q === q);
        if (!cv) throw new Error(`Curve not supported: ${q}`);
        const power = hv.getUint32(4 + n8, true);
        r1 = readerOf(r1csSrc);
        const sr = sectionTable(r1, "r1cs");
        const rh = r1.read(sr[1][0].pos, sr[1][0].len), rv = new DataView(rh.buffer, rh.byteOffset, rh.byteLength);
        const rn8 = rv.getUint32(0, true), prime = leToBig(rh.subarray(4, 4 + rn8));
        const nVars = rv.getUint32(4 + rn8, true), nOutputs = rv.getUint32(8 + rn8, true), nPubInputs = rv.getUint32(12 + rn8, true), nConstraints = rv.getUint32(28 + rn8, true);
        if (prime !== cv.r) throw new SetupRefusal("r1cs curve does not match powers of tau ceremony curve");
        const cirPower = log2(nConstraints + nPubInputs + nOutputs + 1 - 1) + 1;
        if (cirPower > power) throw new SetupRefusal(`circuit too big for this power of tau ceremony. ${nConstraints}*2 > 2**${power}`);
        if (!sp[12]) throw new SetupRefusal("Powers of tau is not prepared.");
        if (cirPower > cv.s) throw new SetupRefusal("Circuit too big for this curve", { throws: true });
        const nPublic = nOutputs + nPubInputs, domainSize = 2 ** cirPower, sG1 = 2 * cv.n8q, sG2 = 4 * cv.n8q;
        const nH = hashedHPoints(domainSize);
        if (domainSize + nH > sp[2][0].len / sG1)
            throw new SetupRefusal(`domainSize 2^${cirPower} equals the ceremony's power: the reference's circuit hash takes H point ${domainSize - 1}, one point past the end of the tauG1 section`,
                                   { handOver: true });
        const alpha1 = pt.read(sp[4][0].pos, sG1), beta1 = pt.read(sp[5][0].pos, sG1), beta2 = pt.read(sp[6][0].pos, sG2);
        const { g1, g2 } = generatorsLem(cv);
        const sec2 = Buffer.concat([u32(cv.n8q, true), bigToLe(cv.q, cv.n8q), u32(32, true), bigToLe(cv.r, 32), u32(nVars, true), u32(nPublic, true), u32(domainSize, true),
                                    alpha1, beta1, beta2, g2, g1, g2]);
        const lag = (id, sz) => pt.read(sp[id][0].pos + (domainSize - 1) * sz, domainSize * sz);
        const dev = addon.groth16Setup(cv.id, nConstraints, nVars, nPublic, domainSize, nH, r1.read(sr[2][0].pos, sr[2][0].len), lag(12, sG1), lag(13, sG2), lag(14, sG1),
                                       lag(15, sG1), pt.read(sp[2][0].pos, (domainSize + nH) * sG1));
        // writeHs (:182-201)
        let sec9;
        if (cirPower < cv.s) {
            const both = pt.read(sp[12][0].pos + (domainSize * 2 - 1) * sG1, domainSize * 2 * sG1);
            sec9 = new Uint8Array(domainSize * sG1);
            for (let i = 0; i < domainSize; i++) sec9.set(both.subarray((i * 2 + 1) * sG1, (i * 2 + 2) * sG1), i * sG1);
        } else sec9 = pt.read(sp[12][0].pos + (2 ** (cirPower + 1) - 1) * sG1 + domainSize * sG1, domainSize * sG1);
        const toU = (group, b) => {
            const n = b.length / (group * sG1), o = new Uint8Array(b.length);
            if (n) addon.groupConvert(cv.id, group, 0, b, o, n);
            return o;
        };
        const hs = crypto.createHash("blake2b512");
        for (const [b, g] of [[alpha1, 1], [beta1, 1], [beta2, 2], [g2, 2], [g1, 1], [g2, 2]]) hs.update(lemToUHost(cv, b, g));
        hs.update(u32(nPublic + 1)); hs.update(toU(1, dev.ic));
        hs.update(u32(domainSize - 1));
        for (const [off, n] of hashHChunks(domainSize)) hs.update(dev.h.subarray(off * sG1, (off + n) * sG1));
        for (const [b, g] of [[dev.c, 1], [dev.a, 1], [dev.b1, 1], [dev.b2, 2]]) { hs.update(u32(b.length / (g * sG1))); hs.update(toU(g, b)); }
        const csHash = new Uint8Array(hs.digest());
        const parts = [Buffer.from("zkey"), u32(1, true), u32(10, true)];
        const sec = (id, body) => { const l = Buffer.alloc(8); l.writeBigUInt64LE(BigInt(body.length)); parts.push(u32(id, true), l, body); };
        sec(1, u32(1, true)); sec(2, sec2); sec(4, dev.coeffs); sec(3, dev.ic); sec(9, sec9); sec(8, dev.c); sec(5, dev.a); sec(6, dev.b1); sec(7, dev.b2);
        sec(10, Buffer.concat([csHash, u32(0, true)]));
        return { zkey: new Uint8Array(Buffer.concat(parts)), csHash };
    } finally {
        pt.close();
        if (r1) r1.close();
    }
}

module.exports = { newZKey, hashHChunks, hashedHPoints, SetupRefusal, CURVES, generatorsLem };
