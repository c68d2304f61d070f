// snarkjs_amd/js/groth16_bellman_native.js — snarkjs.zKey.exportBellman, .bellmanContribute and .importBellman (src/zkey_export_bellman.js,
// src/zkey_bellman_contribute.js, src/zkey_import_bellman.js) through the addon, byte for byte what the reference writes. The twin of
// snarkjs_amd/groth16_bellman.py (DESIGN.md 23):
//   async exportBellman(zkey, options)                                -> { params }
//   async bellmanContribute(curve, challenge, entropy, options)       -> { response, contributionHash }     options.random64: the 64 bytes of getRandomValues
//   async importBellman(zkeyOld, params, name, options)               -> { zkey }
// The H basis change is one addon call each way (bellmanHSection); the other sections go through groupConvert, the 1 / delta of a contribution over H and L
// through ptauChallengeSection (U in, U out). The key pair, hashToG2 and the few header points are host calls of the library. options.dev replaces every
// library call, and its members may return promises (tests/js/bellman_cpu.js: the reference's own curve object in place of the device calls).
// BellmanRefusal: `throws` what the reference throws, `returnsFalse` what it logs with logger.error before it returns false, `handOver` a call left to the
// saved reference function: a file that is not well-formed, a curve or a size this driver does not take, a section beyond one 2^30-byte buffer, an empty
// entropy, a parameter file too short for the sizes it declares (the reference fails there in its own words), a name beyond its length byte.
"use strict";
const crypto = require("crypto"), path = require("path");
const { readerOf, sectionTable } = require("./groth16_native.js");
const p2 = require("./groth16_phase2_native.js");
const setupN = require("./groth16_setup_native.js");
const { formatHash } = require("./groth16_phase2_verify_native.js");

class BellmanRefusal extends Error {
    constructor(message, flags) { super(message); Object.assign(this, flags || {}); }
}
const handOver = (message) => new BellmanRefusal(message, { handOver: true });
const thrown = (message) => new BellmanRefusal(message, { throws: true });
const refusedFalse = (message) => new BellmanRefusal(message, { returnsFalse: true });
const same = (a, b) => a.byteLength == b.byteLength && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;
const u32be = (v) => { const b = Buffer.alloc(4); b.writeUInt32BE(v >>> 0); return b; };
const u32le = (v) => { const b = Buffer.alloc(4); b.writeUInt32LE(v >>> 0); return b; };
const { lemToUHost, leToBig, MAX_SECTION } = p2;

function bigToLe(v, n) { const o = new Uint8Array(n); for (let i = 0; i < n; i++) { o[i] = Number(v & 0xffn); v >>= 8n; } return o; }
function modpow(b, e, m) { let r = 1n; b %= m; while (e > 0n) { if (e & 1n) r = r * b % m; b = b * b % m; e >>= 1n; } return r; }
// batchUtoLEM for a handful of points: the inverse of lemToUHost
function uToLemHost(cv, buf, group) {
    const n8 = cv.n8q, R = 1n << BigInt(8 * n8), el = [];
    for (let o = 0; o < buf.length; o += n8) el.push(bigToLe(BigInt("0x" + Buffer.from(buf.subarray(o, o + n8)).toString("hex")) * R % cv.q, n8));
    return new Uint8Array(Buffer.concat(group == 2 ? el.map((_, i) => el[i ^ 1]) : el));
}

function deviceOf(addon) {
    return {
        // kind 0: LEM -> U, 1: U -> LEM, over a whole section
        convert(cv, group, kind, body) {
            const n = body.byteLength / (2 * group * cv.n8q), out = new Uint8Array(body.byteLength);
            if (n) addon.groupConvert(cv.id, group, kind, Uint8Array.from(body), out, n);
            return out;
        },
        hSection: (cv, body, power, direction) => addon.bellmanHSection(cv.id, Uint8Array.from(body), power, direction),
        // k P for every U-form point of a G1 section, U out
        scaleU(cv, bodyU, k) {
            const n = bodyU.byteLength / (2 * cv.n8q);
            return n ? addon.ptauChallengeSection(cv.id, 1, Uint8Array.from(bodyU), n, Uint8Array.from(k), bigToLe((1n << 256n) % cv.r, 32), 1) : new Uint8Array(0);
        },
        keyFromSeed(cv, seed) {
            const prv = new Uint8Array(32), g1_s = new Uint8Array(2 * cv.n8q), g1_sx = new Uint8Array(2 * cv.n8q);
            addon.call("zkmi_phase2_key_from_seed", cv.id, seed, prv, g1_s, g1_sx);
            return { prv, g1_s, g1_sx };
        },
        hashToG2(cv, transcript) { const o = new Uint8Array(4 * cv.n8q); addon.call("zkmi_phase2_hash_to_g2", cv.id, Uint8Array.from(transcript), o); return o; },
        pointMul(cv, group, point, k) { const o = new Uint8Array(2 * group * cv.n8q); addon.call("zkmi_point_mul", cv.id, group, Uint8Array.from(point), Uint8Array.from(k), o); return o; },
    };
}
const devOf = (options) => options.dev || deviceOf(options.addon || require(path.join(__dirname, "..", "napi", "zkmi_napi.node")));
function open(src) { try { return readerOf(src); } catch (e) { throw handOver(e.message); } }

// readBinFile + readHeader + the bodies a call needs: { cv, sec2, atD1, nVars, nPublic, domainSize, power, body(t), mpc }
function openKey(rd) {
    let tab;
    try { tab = sectionTable(rd, "zkey"); } catch (e) { throw handOver(e.message); }
    const h12 = rd.read(0, 12);
    if (new DataView(h12.buffer, h12.byteOffset, 12).getUint32(4, true) > 2) throw handOver("Version not supported");
    if (!tab[1] || tab[1].length != 1 || tab[1][0].len < 4) throw handOver("section 1 is not there exactly once");
    const protocol = rd.read(tab[1][0].pos, 4);
    if (new DataView(protocol.buffer, protocol.byteOffset, 4).getUint32(0, true) != 1) throw thrown("zkey file is not groth16");
    let end = 12;
    for (const t of Object.keys(tab)) for (const s of tab[t]) {
        if (s.len > MAX_SECTION) throw handOver("a section larger than one buffer");
        end = Math.max(end, s.pos + s.len);
    }
    if (end > rd.size) throw handOver("a section beyond the end of the file");
    for (let t = 2; t <= 10; t++) if (!tab[t] || tab[t].length != 1) throw handOver(`section ${t} is not there exactly once`);
    const sec2 = rd.read(tab[2][0].pos, tab[2][0].len);
    if (sec2.length < 8) throw handOver("a header too short");
    const dv = new DataView(sec2.buffer, sec2.byteOffset, sec2.byteLength), n8q = dv.getUint32(0, true);
    if (sec2.length < 8 + n8q) throw handOver("a header too short");
    const cv = setupN.CURVES.find((c) => c.q === leToBig(sec2.subarray(4, 4 + n8q)));
    if (!cv || cv.n8q != n8q) throw handOver("a curve this driver does not know");
    const n8r = dv.getUint32(4 + n8q, true), at = 8 + n8q + n8r, s1 = 2 * n8q, s2 = 4 * n8q;
    if (sec2.length != at + 12 + 3 * s1 + 3 * s2) throw handOver("a header of an unexpected length");
    const nVars = dv.getUint32(at, true), nPublic = dv.getUint32(at + 4, true), domainSize = dv.getUint32(at + 8, true), power = Math.log2(domainSize);
    if (!Number.isInteger(power) || power < 1 || power + 1 > cv.s || nPublic + 1 > nVars) throw handOver("a domain this driver does not take");
    const want = { 3: (nPublic + 1) * s1, 5: nVars * s1, 6: nVars * s1, 7: nVars * s2, 8: (nVars - nPublic - 1) * s1, 9: domainSize * s1 };
    for (const t of Object.keys(want)) if (tab[t][0].len != want[t]) throw handOver(`section ${t} is not as the header implies`);
    const body = (t) => rd.read(tab[t][0].pos, tab[t][0].len);
    let mpc;
    try {
        mpc = p2.parseMpcParams(body(10), cv);
        if (!same(p2.serialiseMpcParams(mpc), body(10))) throw handOver("section 10 does not serialise back to itself");
    } catch (e) { throw e instanceof BellmanRefusal ? e : handOver(e.message); }
    return { cv, sec2, atD1: at + 12 + 2 * s1 + 2 * s2, nVars, nPublic, domainSize, power, body, mpc };
}
const contributionsU = (cv, list) => list.map((c) => Buffer.concat([lemToUHost(cv, c.deltaAfter, 1), lemToUHost(cv, c.g1_s, 1), lemToUHost(cv, c.g1_sx, 1), lemToUHost(cv, c.g2_spx, 2), Buffer.from(c.transcript)]));

// a parameter file read front to back; a read past its end is the reference's own failure, in its words
class Reader {
    constructor(data) { this.data = data; this.pos = 0; }
    read(n) {
        if (n < 0 || this.pos + n > this.data.length) throw handOver("the parameter file is too short for the sizes it declares");
        this.pos += n;
        return this.data.subarray(this.pos - n, this.pos);
    }
    u32be() { const b = this.read(4); return Buffer.from(b.buffer, b.byteOffset, 4).readUInt32BE(0); }
    contributions(cv) {
        const s1 = 2 * cv.n8q, csHash = this.read(64), n = this.u32be(), out = [];
        if (n > (this.data.length - this.pos) / (5 * s1 + 64)) throw handOver("the parameter file is too short for the sizes it declares");
        for (let i = 0; i < n; i++) {
            const c = {};
            for (const [k, g] of [["deltaAfter", 1], ["g1_s", 1], ["g1_sx", 1], ["g2_spx", 2]]) c[k] = uToLemHost(cv, this.read(s1 * g), g);
            c.transcript = this.read(64);
            out.push(c);
        }
        return { csHash, contributions: out };
    }
}

async function exportBellman(src, options) {
    options = options || {};
    const dev = devOf(options), rd = open(src);
    try {
        const { cv, sec2, atD1, power, body, mpc } = openKey(rd);
        const s1 = 2 * cv.n8q, out = [];
        let at = atD1 - 2 * s1 - 4 * s1;
        for (const group of [1, 1, 2, 2, 1, 2]) { out.push(lemToUHost(cv, sec2.subarray(at, at + s1 * group), group)); at += s1 * group; }
        const points = (group, u) => out.push(u32be(u.byteLength / (s1 * group)), Buffer.from(u.buffer, u.byteOffset, u.byteLength));
        points(1, await dev.convert(cv, 1, 0, body(3)));
        points(1, await dev.hSection(cv, body(9), power, 0));
        for (const [t, group] of [[8, 1], [5, 1], [6, 1], [7, 2]]) points(group, await dev.convert(cv, group, 0, body(t)));
        out.push(Buffer.from(mpc.csHash), u32be(mpc.contributions.length), ...contributionsU(cv, mpc.contributions));
        return { params: new Uint8Array(Buffer.concat(out)) };
    } finally { rd.close(); }
}

async function bellmanContribute(curve, src, entropy, options) {
    options = options || {};
    const log = options.log || (() => {}), dev = devOf(options);
    const name = typeof curve === "string" ? curve.toLowerCase().replace(/[^0-9a-z]/g, "") : (curve && curve.name);
    const cv = setupN.CURVES.find((c) => c.name === ({ bn254: "bn128", altbn128: "bn128" }[name] || name));
    if (!cv) throw handOver("a curve this driver does not know");
    if (!entropy) throw handOver("an empty entropy: the reference asks for one");
    const rd = open(src);
    let data;
    try {
        if (rd.size > MAX_SECTION) throw handOver("a challenge larger than one buffer");
        data = rd.read(0, rd.size);
    } finally { rd.close(); }
    const s1 = 2 * cv.n8q, s2 = 4 * cv.n8q, f = new Reader(data);
    const random64 = options.random64 || crypto.randomBytes(64);
    const head = f.read(2 * s1 + 2 * s2), oldDelta1 = uToLemHost(cv, f.read(s1), 1), oldDelta2 = uToLemHost(cv, f.read(s2), 2);
    const sections = [];
    for (const [what, size] of [["IC", s1], ["H", s1], ["L", s1], ["A", s1], ["B1", s1], ["B2", s2]]) {
        const n = f.u32be();
        if (n > (data.length - f.pos) / size) throw handOver("the parameter file is too short for the sizes it declares");
        sections.push([what, n, f.read(n * size)]);
    }
    const mpc = f.contributions(cv);
    // nothing of the file is left to fail on: the device work starts here
    const key = await dev.keyFromSeed(cv, p2.seedFromEntropy(random64, entropy));
    const R = 1n << 256n, k = leToBig(key.prv) * modpow(R, cv.r - 2n, cv.r) % cv.r, invDelta = bigToLe(modpow(k, cv.r - 2n, cv.r) * R % cv.r, 32);
    const delta1 = await dev.pointMul(cv, 1, oldDelta1, key.prv), delta2 = await dev.pointMul(cv, 2, oldDelta2, key.prv);
    const out = [Buffer.from(head), lemToUHost(cv, delta1, 1), lemToUHost(cv, delta2, 2)];
    for (const [what, n, pts] of sections) {
        const b = what == "H" || what == "L" ? await dev.scaleU(cv, pts, invDelta) : pts;
        out.push(u32be(n), Buffer.from(b.buffer, b.byteOffset, b.byteLength));
    }
    const transcript = crypto.createHash("blake2b512");
    transcript.update(mpc.csHash);
    for (const c of mpc.contributions) p2.hashPubKey(transcript, cv, c);
    transcript.update(lemToUHost(cv, key.g1_s, 1)); transcript.update(lemToUHost(cv, key.g1_sx, 1));
    const cur = { deltaAfter: delta1, g1_s: key.g1_s, g1_sx: key.g1_sx, transcript: new Uint8Array(transcript.digest()), type: 0 };
    cur.g2_spx = await dev.pointMul(cv, 2, await dev.hashToG2(cv, cur.transcript), key.prv);
    mpc.contributions.push(cur);
    out.push(Buffer.from(mpc.csHash), u32be(mpc.contributions.length), ...contributionsU(cv, mpc.contributions));
    const ch = crypto.createHash("blake2b512");
    p2.hashPubKey(ch, cv, cur);
    const contributionHash = new Uint8Array(ch.digest());
    log("info", formatHash(contributionHash, "Contribution Hash: "));
    return { response: new Uint8Array(Buffer.concat(out)), contributionHash };
}

async function importBellman(src, paramsSrc, name, options) {
    options = options || {};
    const dev = devOf(options);
    let rd = open(src), key;
    try { key = openKey(rd); key.kept = {}; for (const t of [3, 4, 5, 6, 7]) key.kept[t] = key.body(t); } finally { rd.close(); }
    const { cv, sec2, atD1, nVars, nPublic, domainSize, power, mpc: old } = key;
    rd = open(paramsSrc);
    let data;
    try {
        if (rd.size > MAX_SECTION) throw handOver("a parameter file larger than one buffer");
        data = rd.read(0, rd.size);
    } finally { rd.close(); }
    const s1 = 2 * cv.n8q, s2 = 4 * cv.n8q;
    // the reference reads the contributions first, at the place the KEY's sizes put them, then the sections front to back
    let f = new Reader(data);
    f.read(3 * s1 + 3 * s2 + 8 + s1 * nVars + 4 + s1 * (domainSize - 1) + 4 + s1 * nVars + 4 + s1 * nVars + 4 + s2 * nVars);
    const neu = f.contributions(cv);
    if (!same(neu.csHash, old.csHash)) throw refusedFalse("Hash of the original circuit does not match with the MPC one");
    if (old.contributions.length > neu.contributions.length) throw refusedFalse("The impoerted file does not include new contributions");
    for (let i = 0; i < old.contributions.length; i++) {
        const a = old.contributions[i], b = neu.contributions[i];
        if (!["deltaAfter", "g1_s", "g1_sx", "g2_spx", "transcript"].every((k) => same(a[k], b[k]))) throw refusedFalse(`Previous contribution ${i} does not match`);
        b.type = a.type;
        for (const k of ["beaconHash", "numIterationsExp", "name"]) if (a[k] !== undefined) b[k] = a[k];
    }
    if (name) for (let i = old.contributions.length; i < neu.contributions.length; i++) neu.contributions[i].name = name;
    let sec10;
    try { sec10 = p2.serialiseMpcParams(neu); } catch (e) { throw e instanceof p2.Phase2Refusal ? handOver(e.message) : e; }
    f = new Reader(data);
    f.read(2 * s1 + 2 * s2);
    const delta1 = uToLemHost(cv, f.read(s1), 1), delta2 = uToLemHost(cv, f.read(s2), 2), taken = {};
    for (const [what, size, want] of [["IC", s1, nPublic + 1], ["H", s1, domainSize - 1], ["L", s1, nVars - nPublic - 1], ["A", s1, nVars], ["B1", s1, nVars], ["B2", s2, nVars]]) {
        if (f.u32be() != want) throw refusedFalse(`Invalid number of points in ${what}`);
        taken[what] = f.read(want * size);
    }
    const h = await dev.hSection(cv, taken.H, power, 1), ell = await dev.convert(cv, 1, 1, taken.L);
    const sections = [[1, u32le(1)], [2, Buffer.concat([Buffer.from(sec2.subarray(0, atD1)), Buffer.from(delta1), Buffer.from(delta2)])], [3, key.kept[3]], [4, key.kept[4]], [9, h], [8, ell],
                      [5, key.kept[5]], [6, key.kept[6]], [7, key.kept[7]], [10, sec10]];
    const parts = [Buffer.from("zkey"), u32le(1), u32le(10)];
    for (const [t, b] of sections) { const hd = Buffer.alloc(12); hd.writeUInt32LE(t); hd.writeBigUInt64LE(BigInt(b.byteLength), 4); parts.push(hd, Buffer.from(b.buffer, b.byteOffset, b.byteLength)); }
    return { zkey: new Uint8Array(Buffer.concat(parts)) };
}

module.exports = { exportBellman, bellmanContribute, importBellman, deviceOf, BellmanRefusal };
