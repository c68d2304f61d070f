// snarkjs_amd/js/groth16_phase2_native.js — snarkjs.zKey.contribute (src/zkey_contribute.js) and zKey.beacon (src/zkey_beacon.js) through the addon:
// contribute(zkey, name, entropy, { random64 }) / beacon(zkey, name, beaconHashStr, numIterationsExp) -> { zkey, contributionHash }, byte for byte the
// reference's key. The twin of snarkjs_amd/groth16_phase2.py. The sections L (8) and H (9) times 1 / delta are one groupScale call each (include/zkmi.h:
// zkmi_group_scale); the key pair, hashToG2 and the header and public-key points are host work in the library (zkmi_phase2_key_from_seed,
// zkmi_phase2_hash_to_g2, zkmi_point_mul); this file hashes (Blake2b-512 and SHA-256 from Node's crypto), reads and writes.
"use strict";
const crypto = require("crypto"), path = require("path");
const { readerOf, sectionTable } = require("./groth16_native.js");

const CURVES = [
    { name: "bn128", id: 0, n8q: 32, q: 21888242871839275222246405745257275088696311157297823662689037894645226208583n,
      r: 21888242871839275222246405745257275088548364400416034343698204186575808495617n },
    { name: "bls12381", id: 1, n8q: 48, q: 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaabn,
      r: 52435875175126190479447740508185965837690552500527637822603658699938581184513n },
];
const MAX_SECTION = 1 << 30;            // one host buffer; a key with a larger L or H section goes to the reference

// what the reference refuses: it throws `message` (throws), or logs it and returns false; handOver: a call left to the reference itself
class Phase2Refusal extends Error {
    constructor(message, flags) { super(message); Object.assign(this, flags || {}); }
}

function leToBig(b) { let v = 0n; for (let i = b.length - 1; i >= 0; i--) v = (v << 8n) | BigInt(b[i]); return v; }
function bigToLe(v, n) { const o = new Uint8Array(n); for (let i = 0; i < n; i++) { o[i] = Number(v & 0xffn); v >>= 8n; } return o; }
function modpow(b, e, m) { let r = 1n; b %= m; while (e > 0n) { if (e & 1n) r = r * b % m; b = b * b % m; e >>= 1n; } return r; }
function u32le(v) { const b = Buffer.alloc(4); b.writeUInt32LE(v >>> 0); return b; }
function lemToUHost(cv, buf, group) {
    const n8 = cv.n8q, rinv = modpow(1n << BigInt(8 * n8), cv.q - 2n, cv.q), el = [];
    for (let o = 0; o < buf.length; o += n8) el.push(bigToLe(leToBig(buf.subarray(o, o + n8)) * rinv % cv.q, n8).reverse());
    return Buffer.concat(group == 2 ? el.map((_, i) => el[i ^ 1]) : el);
}

// zkey_utils.readMPCParams: { csHash, contributions }; points as the affine Montgomery bytes of the file
function parseMpcParams(sec, cv) {
    const s1 = 2 * cv.n8q, s2 = 4 * cv.n8q, dv = new DataView(sec.buffer, sec.byteOffset, sec.byteLength);
    const csHash = sec.subarray(0, 64), n = dv.getUint32(64, true), contributions = [];
    let o = 68;
    for (let i = 0; i < n; i++) {
        const c = { deltaAfter: sec.subarray(o, o + s1), g1_s: sec.subarray(o + s1, o + 2 * s1), g1_sx: sec.subarray(o + 2 * s1, o + 3 * s1), g2_spx: sec.subarray(o + 3 * s1, o + 3 * s1 + s2) };
        o += 3 * s1 + s2;
        c.transcript = sec.subarray(o, o + 64);
        c.type = dv.getUint32(o + 64, true);
        const end = o + 72 + dv.getUint32(o + 68, true);
        o += 72;
        let last = 0;
        while (o < end) {
            const t = sec[o];
            if (t <= last) throw new Phase2Refusal("Parameters in the contribution must be sorted", { throws: true });
            last = t;
            if (t == 1) { c.name = new TextDecoder().decode(sec.subarray(o + 2, o + 2 + sec[o + 1])); o += 2 + sec[o + 1]; }
            else if (t == 2) { c.numIterationsExp = sec[o + 1]; o += 2; }
            else if (t == 3) { c.beaconHash = sec.subarray(o + 2, o + 2 + sec[o + 1]); o += 2 + sec[o + 1]; }
            else throw new Phase2Refusal("Parameter not recognized", { throws: true });
        }
        if (o != end) throw new Phase2Refusal("Parameters do not match", { throws: true });
        contributions.push(c);
    }
    return { csHash, contributions };
}
// zkey_utils.writeMPCParams. The reference writes the name's length into ONE byte, which wraps past 255: such a call is left to the reference.
function serialiseMpcParams(mpc) {
    const out = [Buffer.from(mpc.csHash), u32le(mpc.contributions.length)];
    for (const c of mpc.contributions) {
        out.push(Buffer.from(c.deltaAfter), Buffer.from(c.g1_s), Buffer.from(c.g1_sx), Buffer.from(c.g2_spx), Buffer.from(c.transcript), u32le(c.type || 0));
        const params = [];
        if (c.name) {
            const nameData = new TextEncoder().encode(c.name.substring(0, 64));
            if (nameData.byteLength > 255) throw new Phase2Refusal("name longer than its length field", { handOver: true });
            params.push(1, nameData.byteLength, ...nameData);
        }
        if (c.type == 1) params.push(2, c.numIterationsExp, 3, c.beaconHash.byteLength, ...c.beaconHash);
        out.push(u32le(params.length), Buffer.from(params));
    }
    return Buffer.concat(out);
}
function hashPubKey(h, cv, c) {
    h.update(lemToUHost(cv, c.deltaAfter, 1)); h.update(lemToUHost(cv, c.g1_s, 1)); h.update(lemToUHost(cv, c.g1_sx, 1)); h.update(lemToUHost(cv, c.g2_spx, 2));
    h.update(c.transcript);
}
function seedOf(hash) { const s = new Uint32Array(8); for (let i = 0; i < 8; i++) s[i] = Buffer.from(hash.buffer, hash.byteOffset, hash.byteLength).readUInt32BE(4 * i); return s; }
// misc.getRandomRng: Blake2b-512 over the 64 random bytes and the UTF-8 entropy
function seedFromEntropy(random64, entropy) {
    return seedOf(crypto.createHash("blake2b512").update(random64).update(new TextEncoder().encode(entropy)).digest());
}
// misc.rngFromBeaconParams: 2^numIterationsExp nested SHA-256
function seedFromBeacon(beaconHash, numIterationsExp) {
    let cur = Buffer.from(beaconHash);
    for (let i = 0, n = 2 ** numIterationsExp; i < n; i++) cur = crypto.createHash("sha256").update(cur).digest();
    return seedOf(cur);
}

function apply(zkeySrc, name, seed, extra, options) {
    options = options || {};
    const addon = options.addon || require(path.join(__dirname, "..", "napi", "zkmi_napi.node"));
    const rd = readerOf(zkeySrc);
    try {
        const tab = sectionTable(rd, "zkey");
        const protocol = rd.read(tab[1][0].pos, 4);
        if (new DataView(protocol.buffer, protocol.byteOffset, 4).getUint32(0, true) != 1) throw new Phase2Refusal("zkey file is not groth16", { throws: true });
        if (tab[8][0].len > MAX_SECTION || tab[9][0].len > MAX_SECTION) throw new Phase2Refusal("a point section larger than one buffer", { handOver: true });
        const sec2 = rd.read(tab[2][0].pos, tab[2][0].len), n8q = new DataView(sec2.buffer, sec2.byteOffset, 4).getUint32(0, true);
        const q = leToBig(sec2.subarray(4, 4 + n8q)), cv = CURVES.find((c) => c.q === q);
        if (!cv) throw new Phase2Refusal(`Curve not supported: ${q}`, { throws: true });
        const s1 = 2 * n8q, s2 = 4 * n8q;
        const atD1 = 4 + n8q + 4 + new DataView(sec2.buffer, sec2.byteOffset + 4 + n8q, 4).getUint32(0, true) + 12 + 2 * s1 + 2 * s2;
        const mpc = parseMpcParams(rd.read(tab[10][0].pos, tab[10][0].len), cv);
        const transcript = crypto.createHash("blake2b512");
        transcript.update(mpc.csHash);
        for (const c of mpc.contributions) hashPubKey(transcript, cv, c);
        const prv = new Uint8Array(32), cur = { g1_s: new Uint8Array(s1), g1_sx: new Uint8Array(s1), g2_spx: new Uint8Array(s2) };
        addon.call("zkmi_phase2_key_from_seed", cv.id, seed, prv, cur.g1_s, cur.g1_sx);
        transcript.update(lemToUHost(cv, cur.g1_s, 1)); transcript.update(lemToUHost(cv, cur.g1_sx, 1));
        cur.transcript = new Uint8Array(transcript.digest());
        const g2sp = new Uint8Array(s2);
        addon.call("zkmi_phase2_hash_to_g2", cv.id, cur.transcript, g2sp);
        addon.call("zkmi_point_mul", cv.id, 2, g2sp, prv, cur.g2_spx);
        const delta1 = new Uint8Array(s1), delta2 = new Uint8Array(s2);
        addon.call("zkmi_point_mul", cv.id, 1, Uint8Array.from(sec2.subarray(atD1, atD1 + s1)), prv, delta1);
        addon.call("zkmi_point_mul", cv.id, 2, Uint8Array.from(sec2.subarray(atD1 + s1, atD1 + s1 + s2)), prv, delta2);
        cur.deltaAfter = delta1;
        Object.assign(cur, extra);
        if (name) cur.name = name;
        mpc.contributions.push(cur);
        const sec10 = serialiseMpcParams(mpc);
        const R = 1n << 256n, k = leToBig(prv) * modpow(R, cv.r - 2n, cv.r) % cv.r;
        const invDelta = bigToLe(modpow(k, cv.r - 2n, cv.r) * R % cv.r, 32);
        const scaled = (t) => {
            const body = rd.read(tab[t][0].pos, tab[t][0].len), out = new Uint8Array(body.byteLength);
            if (body.byteLength) addon.groupScale(cv.id, 1, Uint8Array.from(body), out, body.byteLength / s1, invDelta);
            return out;
        };
        const sections = [[1, u32le(1)], [2, Buffer.concat([Buffer.from(sec2.subarray(0, atD1)), Buffer.from(delta1), Buffer.from(delta2)])]];
        for (let t = 3; t <= 7; t++) sections.push([t, Buffer.from(rd.read(tab[t][0].pos, tab[t][0].len))]);
        sections.push([8, Buffer.from(scaled(8))], [9, Buffer.from(scaled(9))], [10, sec10]);
        const parts = [Buffer.from("zkey"), u32le(1), u32le(10)];
        for (const [t, b] of sections) { const h = Buffer.alloc(12); h.writeUInt32LE(t); h.writeBigUInt64LE(BigInt(b.length), 4); parts.push(h, b); }
        const ch = crypto.createHash("blake2b512");
        hashPubKey(ch, cv, cur);
        return { zkey: new Uint8Array(Buffer.concat(parts)), contributionHash: new Uint8Array(ch.digest()), csHash: Uint8Array.from(mpc.csHash) };
    } finally { rd.close(); }
}

function contribute(zkeySrc, name, entropy, options) {
    const random64 = (options && options.random64) || crypto.randomBytes(64);
    return apply(zkeySrc, name, seedFromEntropy(random64, entropy), { type: 0 }, options);
}
// the checks of src/zkey_beacon.js:31-47, in its order and words (the reference logs them and returns false)
function beaconArguments(beaconHashStr, numIterationsExp) {
    let s = beaconHashStr;
    if (s.slice(0, 2) == "0x") s = s.slice(2);
    const beaconHash = new Uint8Array((s.match(/[\da-f]{2}/gi) || []).map((h) => parseInt(h, 16)));
    if (beaconHash.byteLength == 0 || beaconHash.byteLength * 2 != beaconHashStr.length) throw new Phase2Refusal("Invalid Beacon Hash. (It must be a valid hexadecimal sequence)");
    if (beaconHash.length >= 256) throw new Phase2Refusal("Maximum length of beacon hash is 255 bytes");
    numIterationsExp = parseInt(numIterationsExp);
    if (numIterationsExp < 10 || numIterationsExp > 63) throw new Phase2Refusal("Invalid numIterationsExp. (Must be between 10 and 63)");
    return { beaconHash, numIterationsExp };
}
function beacon(zkeySrc, name, beaconHashStr, numIterationsExp, options) {
    const a = beaconArguments(beaconHashStr, numIterationsExp);
    return apply(zkeySrc, name, seedFromBeacon(a.beaconHash, a.numIterationsExp), { type: 1, numIterationsExp: a.numIterationsExp, beaconHash: a.beaconHash }, options);
}

module.exports = { contribute, beacon, Phase2Refusal, parseMpcParams, serialiseMpcParams, seedFromEntropy, seedFromBeacon, hashPubKey, lemToUHost, leToBig, MAX_SECTION };
