// snarkjs_amd/js/powersoftau_challenge_native.js — snarkjs.powersOfTau.exportChallenge, .challengeContribute and .importResponse (src/powersoftau_export_challenge.js,
// src/powersoftau_challenge_contribute.js with applyKeyToChallengeSection of src/mpc_applykey.js, src/powersoftau_import.js) through the addon, byte for byte what
// the reference writes. The twin of snarkjs_amd/powersoftau_challenge.py (DESIGN.md 21):
//   async exportChallenge(ptau, options)                              -> { challenge, challengeHash }
//   async challengeContribute(curve, challenge, entropy, options)     -> { response, responseHash }      options.random64: the 64 bytes of getRandomValues
//   async importResponse(oldPtau, response, name, importPoints, options) -> { ptau, nextChallenge }
// Everything on the points of a section is one addon call: groupConvert(LEM -> U) for the export, ptauChallengeSection (U in, C out) for the response,
// ptauImportSection (C in, LEM and U out) for the import; an import without points takes its recorded points through groupConvert(C -> LEM). The 216 bytes a
// contribution keeps of its response hasher take the reference's cuts (responseCuts): floor(2^24 / sG) points a call with the points, floor(2^24 / scG)
// without. options.log(level, text) receives the reference's info / error lines. options.dev replaces the device calls, which may return promises
// (tests/js/ptau_challenge_cpu.js: the reference's own curve object in their place). ChallengeRefusal: `throws` what the reference throws, `handOver` a call left
// to the saved reference function: a file that is not well-formed, power 0 in importResponse (the reference fails there on its own), a section beyond one
// 2^30-byte buffer, more hasher chunks than the addon's page list takes, an empty entropy, an old section 7 that does not serialise back to itself, a name
// beyond its length byte, a curve this driver does not know.
"use strict";
const crypto = require("crypto"), path = require("path");
const { readerOf, sectionTable } = require("./groth16_native.js");
const { seedFromEntropy, lemToUHost, leToBig, MAX_SECTION } = require("./groth16_phase2_native.js");
const setupN = require("./groth16_setup_native.js");
const { formatHash } = require("./groth16_phase2_verify_native.js");
const prepareN = require("./powersoftau_prepare_native.js");
const verifyN = require("./powersoftau_verify_native.js");
const contribN = require("./powersoftau_contribute_native.js");

class ChallengeRefusal extends Error {
    constructor(message, flags) { super(message); Object.assign(this, flags || {}); }
}
const handOver = (message) => new ChallengeRefusal(message, { handOver: true });
const thrown = (message) => new ChallengeRefusal(message, { throws: true });
const CORRUPTED = "PTau file is corrupted. Calculated new challenge hash does not match with the eclared one";
const MAX_CHUNKS = 256;                 // pages of one addon argument
const KEYS = ["tau", "alpha", "beta"];
const KEY_FIELDS = [["tau.g1_s", 1], ["tau.g1_sx", 1], ["alpha.g1_s", 1], ["alpha.g1_sx", 1], ["beta.g1_s", 1], ["beta.g1_sx", 1], ["tau.g2_spx", 2], ["alpha.g2_spx", 2], ["beta.g2_spx", 2]];
const same = (a, b) => a.byteLength == b.byteLength && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;
const blake = (...parts) => { const h = crypto.createHash("blake2b512"); for (const p of parts) h.update(p); return new Uint8Array(h.digest()); };
const shapes = (power) => [[2, 1, 2 * 2 ** power - 1], [3, 2, 2 ** power], [4, 1, 2 ** power], [5, 1, 2 ** power], [6, 2, 1]];

function deviceOf(addon) {
    return Object.assign(contribN.deviceOf(addon), {
        // kind 0: LEM -> U, 3: C -> LEM
        convert(cv, group, kind, body, n) {
            const out = new Uint8Array(n * 2 * group * cv.n8q);
            if (n) addon.groupConvert(cv.id, group, kind, body, out, n);
            return out;
        },
        // bodyU: the n U-form points of a challenge section; first, inc: Montgomery Fr bytes -> the C bytes of (first * inc^i) P_i
        challengeSection: (cv, group, bodyU, n, first, inc) => addon.ptauChallengeSection(cv.id, group, bodyU, n, Uint8Array.from(first), Uint8Array.from(inc), 0),
        importSection(cv, group, bodyC, n) {
            const b = n * 2 * group * cv.n8q, r = addon.ptauImportSection(cv.id, group, bodyC, n);
            return { lem: r.subarray(0, b), u: r.subarray(b) };
        },
    });
}

// the byte lengths of the update calls importResponse makes on its response hasher before it takes the partial hash
function responseCuts(cv, power, importPoints) {
    const cuts = [64];
    for (const [, group, n] of shapes(power)) {
        const sc = group * cv.n8q, per = Math.floor((1 << 24) / (importPoints ? 2 * sc : sc));
        for (let i = 0; i < n; i += per) cuts.push(Math.min(per, n - i) * sc);
    }
    return cuts;
}

// batchUtoLEM for the nine points of a public key: the inverse of lemToUHost
function uToLemHost(cv, buf, group) {
    const n8 = cv.n8q, R = 1n << BigInt(8 * n8), el = [];
    for (let o = 0; o < buf.length; o += n8) {
        let v = BigInt("0x" + Buffer.from(buf.subarray(o, o + n8)).toString("hex")) * R % cv.q;
        const b = new Uint8Array(n8);
        for (let i = 0; i < n8; i++) { b[i] = Number(v & 0xffn); v >>= 8n; }
        el.push(b);
    }
    return new Uint8Array(Buffer.concat(group == 2 ? el.map((_, i) => el[i ^ 1]) : el));
}

// readBinFile + readPTauHeader for a file that may hold sections 1 and 7 alone
function openHeader(rd) {
    let tab;
    try { tab = sectionTable(rd, "ptau"); } catch (e) { throw handOver(e.message); }
    const h12 = rd.read(0, 12);
    if (new DataView(h12.buffer, h12.byteOffset, 12).getUint32(4, true) > 1) throw handOver("Version not supported");
    let end = 12;
    for (const t of Object.keys(tab)) for (const s of tab[t]) {
        if (s.len > MAX_SECTION) throw handOver("a section larger than one buffer");
        end = Math.max(end, s.pos + s.len);
    }
    if (end > rd.size) throw handOver("a section beyond the end of the file");
    for (const t of [1, 7]) if (!tab[t] || tab[t].length != 1) throw handOver(`section ${t} is not there exactly once`);
    const head = rd.read(tab[1][0].pos, tab[1][0].len);
    if (head.length < 4) throw handOver("Invalid PTau header size");
    const hv = new DataView(head.buffer, head.byteOffset, head.byteLength), n8 = hv.getUint32(0, true);
    if (head.length != 4 + n8 + 8) throw handOver("Invalid PTau header size");
    const q = leToBig(head.subarray(4, 4 + n8)), cv = setupN.CURVES.find((c) => c.q === q);
    if (!cv || cv.n8q != n8) throw handOver("Curve not supported");
    const power = hv.getUint32(4 + n8, true);
    if (power + 1 > cv.s) throw handOver("power + 1 > Fr.s");
    return { tab, cv, power, head };
}
function contributionsOf(rd, tab, cv, dev) {
    const old7 = rd.read(tab[7][0].pos, tab[7][0].len);
    let contributions;
    try { contributions = verifyN.readContributions(cv, old7, dev); } catch (e) { throw e instanceof verifyN.PtauRefusal ? handOver(e.message) : e; }
    if (!same(contribN.writeContributions(cv, contributions), old7)) throw handOver("the contributions of the old file do not serialise back to its section 7");
    return contributions;
}
const devOf = (options) => options.dev || deviceOf(options.addon || require(path.join(__dirname, "..", "napi", "zkmi_napi.node")));
function open(src) { try { return readerOf(src); } catch (e) { throw handOver(e.message); } }

async function exportChallenge(src, options) {
    options = options || {};
    const log = options.log || (() => {}), dev = devOf(options);
    const rd = open(src);
    try {
        const { tab, cv, power } = openHeader(rd);
        const contributions = contributionsOf(rd, tab, cv, dev);
        const last = contributions.length ? contributions[contributions.length - 1] : null;
        const lastResponse = last ? last.responseHash : blake(), declared = last ? last.nextChallenge : verifyN.firstChallengeHash(cv, power);
        // a file imported without points: the reference has logged its two lines when startReadUniqueSection throws, with the file's name in front
        for (const [t, group, n] of shapes(power)) if (tab[t] && (tab[t].length != 1 || tab[t][0].len < n * 2 * group * cv.n8q)) throw handOver(`section ${t} is not as the header implies`);
        log("info", formatHash(lastResponse, "Last Response Hash: "));
        log("info", formatHash(declared, "New Challenge Hash: "));
        const out = [Buffer.from(lastResponse)];
        for (const [t, group, n] of shapes(power)) {
            if (!tab[t]) throw thrown(`${options.fileName}: Missing section ${t}`);
            out.push(await dev.convert(cv, group, 0, rd.read(tab[t][0].pos, n * 2 * group * cv.n8q), n));
        }
        const challenge = new Uint8Array(Buffer.concat(out)), calc = blake(challenge);
        if (!same(calc, declared)) {
            log("info", formatHash(calc, "Calc Curret Challenge Hash: "));
            log("error", CORRUPTED);
            throw new ChallengeRefusal(CORRUPTED, { throws: true, challenge });                  // the reference has written the file by then
        }
        return { challenge, challengeHash: new Uint8Array(declared) };
    } finally { rd.close(); }
}

async function challengeContribute(curve, src, entropy, options) {
    options = options || {};
    const log = options.log || (() => {}), dev = devOf(options);
    const name = typeof curve === "string" ? curve.toLowerCase().replace(/[^0-9a-z]/g, "") : (curve && curve.name);
    const cv = setupN.CURVES.find((c) => c.name === ({ bn254: "bn128", altbn128: "bn128" }[name] || name));
    if (!cv) throw handOver("a curve this driver does not know");
    const rd = open(src);
    try {
        const s1 = 2 * cv.n8q, s2 = 4 * cv.n8q, domain = (rd.size + s1 - 64 - s2) / (4 * s1 + s2);
        let e = domain, power = 0;
        while (e > 1) { e = e / 2; power += 1; }
        if (2 ** power != domain) throw thrown("Invalid file size");
        if (!entropy) throw handOver("an empty entropy: the reference asks for one");
        if (rd.size > MAX_SECTION) throw handOver("a challenge larger than one buffer");
        const random64 = options.random64 || crypto.randomBytes(64);
        const data = rd.read(0, rd.size);
        log("info", formatHash(data.subarray(0, 64), "Claimed Previous Response Hash: "));
        const challengeHash = blake(data);
        log("info", formatHash(challengeHash, "Current Challenge Hash: "));
        const k = dev.ptauKeyFromSeed(cv, seedFromEntropy(random64, entropy)), key = {};
        for (let i = 0; i < 3; i++) {
            key[`${KEYS[i]}.g1_s`] = k.s[i]; key[`${KEYS[i]}.g1_sx`] = k.sx[i];
            key[`${KEYS[i]}.g2_spx`] = dev.pointMul(cv, 2, verifyN.g2sp(dev, cv, i, challengeHash, k.s[i], k.sx[i]), k.prv[i]);
        }
        const [tau, alpha, beta] = k.prv;
        const one = Buffer.from(((1n << 256n) % cv.r).toString(16).padStart(64, "0"), "hex").reverse();
        const out = [Buffer.from(challengeHash)], firsts = [one, one, alpha, beta, beta];
        let at = 64, i = 0;
        for (const [, group, n] of shapes(power)) {
            const size = n * 2 * group * cv.n8q;
            out.push(await dev.challengeSection(cv, group, data.subarray(at, at + size), n, firsts[i++], tau));
            at += size;
        }
        for (const [f, g] of KEY_FIELDS) out.push(lemToUHost(cv, key[f], g));                     // toPtauPubKeyRpr(..., false): normal-form U bytes
        const response = new Uint8Array(Buffer.concat(out)), responseHash = blake(response);
        log("info", formatHash(responseHash, "Contribution Response Hash: "));
        return { response, responseHash };
    } finally { rd.close(); }
}

async function importResponse(src, responseSrc, name, importPoints, options) {
    options = options || {};
    const log = options.log || (() => {}), dev = devOf(options);
    let rd = open(src), tab, cv, power, head, contributions;
    try {
        ({ tab, cv, power, head } = openHeader(rd));
        contributions = contributionsOf(rd, tab, cv, dev);
    } finally { rd.close(); }
    rd = open(responseSrc);
    let data;
    try {
        const n8 = cv.n8q, s1 = 2 * n8, s2 = 4 * n8;
        let want = 64 + 6 * s1 + 3 * s2;
        for (const [, group, n] of shapes(power)) want += n * group * n8;
        if (rd.size != want) throw thrown("Size of the contribution is invalid");
        if (rd.size > MAX_SECTION) throw handOver("a response larger than one buffer");
        data = rd.read(0, rd.size);
    } finally { rd.close(); }
    const n8 = cv.n8q;
    let last = contributions.length ? contributions[contributions.length - 1].nextChallenge : verifyN.firstChallengeHash(cv, power);
    const previous = data.subarray(0, 64);
    if (last.every((b) => b === 0xff)) {
        if (!contributions.length) throw handOver("no contribution to take the response's previous hash: the reference fails on it");
        last = Uint8Array.from(previous);
        contributions[contributions.length - 1].nextChallenge = last;
    }
    if (!same(previous, last)) throw thrown("Wrong contribution. This contribution is not based on the previous hash");
    if (power == 0) throw handOver("power 0");
    const cur = {};
    if (name) cur.name = name;
    const secs = [[1, [prepareN.headerOf(head, cv, power)]]], us = [], fields = ["tauG1", "tauG2", "alphaG1", "betaG1", "betaG2"], sp = [1, 1, 0, 0, 0];
    let at = 64, i = 0;
    for (const [t, group, n] of shapes(power)) {
        const sc = group * n8, sg = 2 * sc, body = data.subarray(at, at + n * sc), s = sp[i], field = fields[i++];
        at += n * sc;
        if (importPoints) {
            if (n * sg > MAX_SECTION) throw handOver("a section larger than one buffer");
            const r = await dev.importSection(cv, group, body, n);
            secs.push([t, [r.lem]]);
            us.push(r.u);
            cur[field] = r.lem.subarray(s * sg, (s + 1) * sg);
        } else cur[field] = await dev.convert(cv, group, 3, Uint8Array.from(body.subarray(s * sc, (s + 1) * sc)), 1);
    }
    const cuts = responseCuts(cv, power, importPoints), chunks = [];
    if (cuts.length > MAX_CHUNKS) throw handOver("more chunks of the response hasher than one addon call takes");
    let o = 0;
    for (const ln of cuts) { chunks.push(data.subarray(o, o + ln)); o += ln; }
    cur.partialHash = await dev.blake2bPartial(chunks);
    cur.key = {};
    for (const [f, g] of KEY_FIELDS) { cur.key[f] = uToLemHost(cv, data.subarray(at, at + 2 * g * n8), g); at += 2 * g * n8; }
    const responseHash = blake(data);
    log("info", formatHash(responseHash, "Contribution Response Hash imported: "));
    if (importPoints) {
        cur.nextChallenge = blake(responseHash, ...us);
        log("info", formatHash(cur.nextChallenge, "Next Challenge Hash: "));
    } else cur.nextChallenge = new Uint8Array(64).fill(0xff);
    secs.push([7, [contribN.writeContributions(cv, contributions.concat([cur]))]]);
    return { ptau: prepareN.fileOf(secs), nextChallenge: cur.nextChallenge };
}

module.exports = { exportChallenge, challengeContribute, importResponse, deviceOf, responseCuts, ChallengeRefusal };
