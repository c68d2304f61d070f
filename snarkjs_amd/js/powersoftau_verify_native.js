// snarkjs_amd/js/powersoftau_verify_native.js — snarkjs.powersOfTau.verify (src/powersoftau_verify.js) through the addon: async verify(ptau, { log, random32 })
// -> true | false, with log(level, text) receiving the reference's info / warn / error lines in its order (its debug progress lines are not reproduced). The
// twin of snarkjs_amd/powersoftau_verify.py (DESIGN.md 18). Everything on curve points is ptauSectionCheck, once per section 2 - 5 from one upload (the section
// in U form for the hash, the two sums of processSection, one verdict per power of verifyLagrangeEvaluations), and ONE sameRatioBatch of all 8 c + 4 checks of a
// file with c contributions; the host work of all contributions is done first. random32: seed j is the first 32 bytes of blake2b(random32 || byte j), j = 2 .. 5
// the pair seeds, 12 .. 15 the ladder seeds. options.dev replaces the device calls, which may return promises (tests/js/ptau_verify_cpu.js: the reference's own
// curve in their place). Handed to the saved reference function (PtauRefusal.handOver): a section beyond one 2^30-byte buffer, power + 1 > Fr.s, inputs the
// readers do not take.
"use strict";
const crypto = require("crypto"), path = require("path");
const { readerOf, sectionTable } = require("./groth16_native.js");
const { seedFromBeacon, lemToUHost, leToBig, MAX_SECTION } = require("./groth16_phase2_native.js");
const setupN = require("./groth16_setup_native.js");
const { formatHash } = require("./groth16_phase2_verify_native.js");

// what the reference throws (throws), or a call left to the reference itself (handOver)
class PtauRefusal extends Error {
    constructor(message, flags) { super(message); Object.assign(this, flags || {}); }
}
const same = (a, b) => a.byteLength == b.byteLength && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;
const blake = (...bufs) => { const h = crypto.createHash("blake2b512"); for (const b of bufs) h.update(b); return h.digest(); };
function seedBytes(b32) {
    const w = new Uint32Array(8), b = Buffer.from(b32.buffer, b32.byteOffset, 32);
    for (let i = 0; i < 8; i++) w[i] = b.readUInt32BE(4 * i);
    return new Uint8Array(w.buffer);
}

function deviceOf(addon) {
    const affine = (cv, group, jac) => { const out = new Uint8Array(2 * group * cv.n8q); addon.call("zkmi_to_affine", cv.id, group, Uint8Array.from(jac), out); return out; };
    return {
        sectionCheck(cv, group, tau, nTau, lagrange, top, zeroLast, pairSeed32, ladderSeed32) {
            const sg = 2 * group * cv.n8q, jac = 3 * group * cv.n8q, ub = nTau * sg;
            const r = addon.ptauSectionCheck(cv.id, group, tau, nTau, lagrange, top, zeroLast ? 1 : 0, seedBytes(pairSeed32), seedBytes(ladderSeed32));
            return { u: r.subarray(0, ub), r1: affine(cv, group, r.subarray(ub, ub + jac)), r2: affine(cv, group, r.subarray(ub + jac, ub + 2 * jac)),
                     ladder: lagrange ? Array.from(r.subarray(ub + 2 * jac), (v) => v === 1) : null };
        },
        sameRatioBatch(cv, checks) {
            if (!checks.length) return [];
            const cols = [0, 1, 2, 3].map((k) => new Uint8Array(Buffer.concat(checks.map((c) => Buffer.from(c[k])))));
            return Array.from(addon.sameRatioBatch(cv.id, cols[0], cols[1], cols[2], cols[3], checks.length), (v) => v === 1);
        },
        blake2bResume: (partial, data) => addon.blake2bResume(Uint8Array.from(partial), Uint8Array.from(data)),
        hashToG2(cv, h64) { const out = new Uint8Array(4 * cv.n8q); addon.call("zkmi_phase2_hash_to_g2", cv.id, Uint8Array.from(h64), out); return out; },
        // keypair.createPTauKey up to its G2 halves: { prv: [3 x 32 bytes], s: [3 points], sx: [3 points] }
        ptauKeyFromSeed(cv, seed) {
            const s1 = 2 * cv.n8q, prv = new Uint8Array(96), s = new Uint8Array(3 * s1), sx = new Uint8Array(3 * s1);
            addon.call("zkmi_ptau_key_from_seed", cv.id, seed, prv, s, sx);
            const cut = (b, n) => [0, 1, 2].map((i) => b.subarray(i * n, (i + 1) * n));
            return { prv: cut(prv, 32), s: cut(s, s1), sx: cut(sx, s1) };
        },
        pointMul(cv, group, p, k) { const out = new Uint8Array(2 * group * cv.n8q); addon.call("zkmi_point_mul", cv.id, group, Uint8Array.from(p), Uint8Array.from(k), out); return out; },
    };
}

const KEYS = ["tau", "alpha", "beta"];
// powersoftau_utils.readContributions on the bytes of section 7
function readContributions(cv, body, dev) {
    const s1 = 2 * cv.n8q, s2 = 4 * cv.n8q, dv = new DataView(body.buffer, body.byteOffset, body.byteLength), out = [];
    const bad = () => new PtauRefusal("Invalid contribution section size", { throws: true });
    if (body.length < 4) throw bad();
    let o = 4;
    for (let i = 0, n = dv.getUint32(0, true); i < n; i++) {
        const c = { id: i + 1, key: {} };
        if (o + 3 * s1 + 2 * s2 + 6 * s1 + 3 * s2 + 288 > body.length) throw bad();
        for (const [k, sz] of [["tauG1", s1], ["tauG2", s2], ["alphaG1", s1], ["betaG1", s1], ["betaG2", s2]]) { c[k] = body.subarray(o, o + sz); o += sz; }
        for (const k of KEYS) for (const f of ["g1_s", "g1_sx"]) { c.key[`${k}.${f}`] = body.subarray(o, o + s1); o += s1; }
        for (const k of KEYS) { c.key[`${k}.g2_spx`] = body.subarray(o, o + s2); o += s2; }
        c.partialHash = body.subarray(o, o + 216); c.nextChallenge = body.subarray(o + 216, o + 280);
        c.type = dv.getUint32(o + 280, true);
        const end = o + 288 + dv.getUint32(o + 284, true);
        o += 288;
        let last = 0;
        while (o < end) {
            const typ = body[o];
            if (typ <= last) throw new PtauRefusal("Parameters in the contribution must be sorted", { throws: true });
            last = typ;
            if (typ == 1) { c.name = new TextDecoder().decode(body.subarray(o + 2, o + 2 + body[o + 1])); o += 2 + body[o + 1]; }
            else if (typ == 2) { c.numIterationsExp = body[o + 1]; o += 2; }
            else if (typ == 3) { c.beaconHash = body.subarray(o + 2, o + 2 + body[o + 1]); o += 2 + body[o + 1]; }
            else throw new PtauRefusal("Parameter not recognized", { throws: true });
        }
        if (o != end) throw new PtauRefusal("Parameters do not match", { throws: true });
        const pub = [];
        for (const k of KEYS) for (const f of ["g1_s", "g1_sx"]) pub.push(lemToUHost(cv, c.key[`${k}.${f}`], 1));
        for (const k of KEYS) pub.push(lemToUHost(cv, c.key[`${k}.g2_spx`], 2));
        c.responseHash = dev.blake2bResume(c.partialHash, Buffer.concat(pub));
        out.push(c);
    }
    if (o != body.length) throw bad();
    return out;
}

// powersoftau_utils.calculateFirstChallengeHash: the generators repeated, fed from one buffer
function firstChallengeHash(cv, ceremonyPower) {
    const { g1, g2 } = setupN.generatorsLem(cv), u1 = lemToUHost(cv, g1, 1), u2 = lemToUHost(cv, g2, 2);
    const h = crypto.createHash("blake2b512");
    h.update(crypto.createHash("blake2b512").digest());
    const block = (u, n) => {
        const big = Buffer.concat(Array.from({ length: Math.min(n, 1 << 14) }, () => u));
        for (let i = 0; i < Math.floor(n / (1 << 14)); i++) h.update(big);
        h.update(big.subarray(0, (n % (1 << 14)) * u.length));
    };
    const n = 2 ** ceremonyPower;
    block(u1, 2 * n - 1); block(u2, n); block(u1, n); block(u1, n);
    h.update(u2);
    return h.digest();
}

// keypair.getG2sp
const g2sp = (dev, cv, pers, challenge, s, sx) => dev.hashToG2(cv, blake(Buffer.from([pers]), challenge, lemToUHost(cv, s, 1), lemToUHost(cv, sx, 1)));

// the first of the nine comparisons of a beacon contribution's key that fails, as the reference names it (null: all hold)
function beaconFailure(dev, cv, cur, prev) {
    if (!cur.beaconHash || cur.numIterationsExp === undefined) throw new PtauRefusal(`beacon contribution #${cur.id} has no beaconHash or numIterationsExp parameter`, { throws: true });
    const k = dev.ptauKeyFromSeed(cv, seedFromBeacon(cur.beaconHash, cur.numIterationsExp));
    for (let i = 0; i < 3; i++) {
        if (!same(cur.key[`${KEYS[i]}.g1_s`], k.s[i])) return `${KEYS[i]}G1_s`;
        if (!same(cur.key[`${KEYS[i]}.g1_sx`], k.sx[i])) return `${KEYS[i]}G1_sx`;
        if (!same(cur.key[`${KEYS[i]}.g2_spx`], dev.pointMul(cv, 2, g2sp(dev, cv, i, prev.nextChallenge, k.s[i], k.sx[i]), k.prv[i]))) return `${KEYS[i]}G2_spx`;
    }
    return null;
}

const RATIO_LINES = [(id) => `INVALID key (tau) in challenge #${id}`, (id) => `INVALID key (alpha) in challenge #${id}`, (id) => `INVALID key (beta) in challenge #${id}`,
    (id) => `INVALID tau*G1. challenge #${id} It does not follow the previous contribution`, (id) => `INVALID tau*G2. challenge #${id} It does not follow the previous contribution`,
    (id) => `INVALID alpha*G1. challenge #${id} It does not follow the previous contribution`, (id) => `INVALID beta*G1. challenge #${id} It does not follow the previous contribution`,
    (id) => `INVALID beta*G2. challenge #${id}It does not follow the previous contribution`];

// the eight sameRatio calls of verifyContribution, in its order
function contributionChecks(dev, cv, cur, prev) {
    const k = cur.key, sp = KEYS.map((n, i) => g2sp(dev, cv, i, prev.nextChallenge, k[`${n}.g1_s`], k[`${n}.g1_sx`]));
    return [[k["tau.g1_s"], k["tau.g1_sx"], sp[0], k["tau.g2_spx"]], [k["alpha.g1_s"], k["alpha.g1_sx"], sp[1], k["alpha.g2_spx"]], [k["beta.g1_s"], k["beta.g1_sx"], sp[2], k["beta.g2_spx"]],
            [prev.tauG1, cur.tauG1, sp[0], k["tau.g2_spx"]], [k["tau.g1_s"], k["tau.g1_sx"], prev.tauG2, cur.tauG2], [prev.alphaG1, cur.alphaG1, sp[1], k["alpha.g2_spx"]],
            [prev.betaG1, cur.betaG1, sp[2], k["beta.g2_spx"]], [k["beta.g1_s"], k["beta.g1_sx"], prev.betaG2, cur.betaG2]];
}

async function verify(src, options) {
    options = options || {};
    const log = options.log || (() => {});
    const dev = options.dev || deviceOf(options.addon || require(path.join(__dirname, "..", "napi", "zkmi_napi.node")));
    const random32 = options.random32 || crypto.randomBytes(32);
    const seedOf = (j) => new Uint8Array(blake(random32, Buffer.from([j]))).subarray(0, 32);
    let rd;
    try { rd = readerOf(src); } catch (e) { throw new PtauRefusal(e.message, { handOver: true }); }
    try {
        const tab = sectionTable(rd, "ptau");
        if (!tab[1]) throw new PtauRefusal("File has no  header", { throws: true });
        if (tab[1].length > 1) throw new PtauRefusal("File has more than one header", { throws: true });
        for (const t of Object.keys(tab)) for (const s of tab[t]) if (s.len > MAX_SECTION) throw new PtauRefusal("a section larger than one buffer", { handOver: true });
        const head = rd.read(tab[1][0].pos, tab[1][0].len), hv = new DataView(head.buffer, head.byteOffset, head.byteLength), n8 = hv.getUint32(0, true);
        if (head.length != 4 + n8 + 8) throw new PtauRefusal("Invalid PTau header size", { throws: true });
        const q = leToBig(head.subarray(4, 4 + n8)), cv = setupN.CURVES.find((c) => c.q === q);
        if (!cv) throw new PtauRefusal(`Curve not supported: ${q}`, { throws: true });
        const power = hv.getUint32(4 + n8, true), ceremonyPower = hv.getUint32(8 + n8, true);
        if (power + 1 > cv.s) throw new PtauRefusal("power + 1 > Fr.s", { handOver: true });
        if (!tab[7]) throw new PtauRefusal("File has no  contributions", { throws: true });
        const contrs = readContributions(cv, rd.read(tab[7][0].pos, tab[7][0].len), dev);
        if (!contrs.length) { log("error", "This file has no contribution! It cannot be used in production"); return false; }
        const s2 = 4 * cv.n8q, { g1, g2 } = setupN.generatorsLem(cv);

        // the host work of all contributions, last to first as they are reported
        const initial = { tauG1: g1, tauG2: g2, alphaG1: g1, betaG1: g1, betaG2: g2 }, checks = [], beaconBad = {};
        for (let i = contrs.length - 1; i >= 0; i--) {
            const cur = contrs[i];
            if (i == 0) initial.nextChallenge = firstChallengeHash(cv, ceremonyPower);
            const prev = i ? contrs[i - 1] : initial;
            if (cur.type == 1) {
                const bad = beaconFailure(dev, cv, cur, prev);
                if (bad) { beaconBad[i] = bad; break; }                                     // nothing after this failure is reported
            }
            checks.push(...contributionChecks(dev, cv, cur, prev));
        }
        // the four sections, one call each; what the reference throws at a section is thrown where it would reach that section
        const last = contrs[contrs.length - 1], lagrangeThere = [12, 13, 14, 15].every((t) => tab[t]);
        const hasher = crypto.createHash("blake2b512"), sec = {}, secThrow = {};
        hasher.update(last.responseHash);
        for (const [t, group, nTau, top] of [[2, 1, 2 * 2 ** power - 1, power + 1], [3, 2, 2 ** power, power], [4, 1, 2 ** power, power], [5, 1, 2 ** power, power]]) {
            const sg = 2 * group * cv.n8q, lagLen = (2 * 2 ** top - 1) * sg;
            if (!tab[t]) secThrow[t] = `ptau: Missing section ${t}`;
            else if (tab[t].length > 1) secThrow[t] = `ptau: Section Duplicated ${t}`;
            else if (tab[t][0].len != nTau * sg) secThrow[t] = "Invalid section size reading";
            if (secThrow[t]) break;
            const lagOk = lagrangeThere && tab[t + 10].length == 1 && tab[t + 10][0].len >= lagLen;
            const tau = rd.read(tab[t][0].pos, tab[t][0].len), lag = lagOk ? rd.read(tab[t + 10][0].pos, lagLen) : null;
            const r = await dev.sectionCheck(cv, group, tau, nTau, lag, top, t == 2, seedOf(t), seedOf(t + 10));
            hasher.update(r.u);
            sec[t] = { first: tau.subarray(0, sg), second: tau.subarray(sg, 2 * sg), r1: r.r1, r2: r.r2, ladder: r.ladder,
                       lagThrow: lagrangeThere && !lagOk ? (tab[t + 10].length > 1 ? `ptau: Section Duplicated ${t + 10}` : "Invalid section size reading") : null };
        }
        const betaG2 = tab[6] && tab[6].length == 1 ? rd.read(tab[6][0].pos, s2) : null;
        const at = {};
        for (const [t, c] of [[2, (s) => [s.r1, s.r2, g2, last.tauG2]], [3, (s) => [g1, last.tauG1, s.r1, s.r2]], [4, (s) => [s.r1, s.r2, g2, last.tauG2]], [5, (s) => [s.r1, s.r2, g2, last.tauG2]]])
            if (sec[t]) { at[t] = checks.length; checks.push(c(sec[t])); }
        const verdicts = await dev.sameRatioBatch(cv, checks);

        // the lines, in the reference's order
        const contributionOk = (i) => {
            const cur = contrs[i];
            if (beaconBad[i]) { log("error", `BEACON key (${beaconBad[i]}) is not generated correctly in challenge #${cur.id}  ${cur.name || ""}`); return false; }
            for (let j = 0; j < 8; j++) if (!verdicts[8 * (contrs.length - 1 - i) + j]) { log("error", RATIO_LINES[j](cur.id)); return false; }
            log("info", "Powers Of tau file OK!");
            return true;
        };
        const printContribution = (i) => {
            const cur = contrs[i], prev = i ? contrs[i - 1] : initial;
            log("info", "-----------------------------------------------------");
            log("info", `Contribution #${cur.id}: ${cur.name || ""}`);
            log("info", formatHash(cur.nextChallenge, "Next Challenge: "));
            log("info", formatHash(cur.responseHash, "Response Hash:"));
            log("info", formatHash(prev.nextChallenge, "Response Hash:"));
            if (cur.type == 1) {
                log("info", `Beacon generator: ${Buffer.from(cur.beaconHash).toString("hex")}`);
                log("info", `Beacon iterations Exp: ${cur.numIterationsExp}`);
            }
        };
        if (!contributionOk(contrs.length - 1)) return false;
        for (const [t, name, firsts] of [
            [2, "tauG1", [[g1, "First element of tau*G1 section must be the generator"], [last.tauG1, "Second element of tau*G1 section does not match the one in the contribution section"]]],
            [3, "tauG2", [[g2, "First element of tau*G2 section must be the generator"], [last.tauG2, "Second element of tau*G2 section does not match the one in the contribution section"]]],
            [4, "alphaTauG1", [[last.alphaG1, "First element of alpha*tau*G1 section (alpha*G1) does not match the one in the contribution section"]]],
            [5, "betaTauG1", [[last.betaG1, "First element of beta*tau*G1 section (beta*G1) does not match the one in the contribution section"]]]]) {
            if (secThrow[t]) throw new PtauRefusal(secThrow[t], { throws: true });
            if (!verdicts[at[t]]) { log("error", `${name} section. Powers do not match`); return false; }
            const got = [sec[t].first, sec[t].second];
            for (let j = 0; j < firsts.length; j++) if (!same(got[j], firsts[j][0])) { log("error", firsts[j][1]); return false; }
        }
        if (!betaG2) {
            log("error", "File has no BetaG2 section");
            throw new PtauRefusal(tab[6] ? "File has more than one GetaG2 section" : "File has no BetaG2 section", { throws: true });
        }
        hasher.update(lemToUHost(cv, betaG2, 2));
        if (!same(betaG2, last.betaG2)) { log("error", "betaG2 element in betaG2 section does not match the one in the contribution section"); return false; }
        const nextHash = hasher.digest();
        if (power == ceremonyPower && !same(nextHash, last.nextChallenge)) {
            log("error", "Hash of the values does not match the next challenge of the last contributor in the contributions section");
            return false;
        }
        log("info", formatHash(nextHash, "Next challenge hash: "));
        printContribution(contrs.length - 1);
        for (let i = contrs.length - 2; i >= 0; i--) {
            if (!contributionOk(i)) return false;
            printContribution(i);
        }
        log("info", "-----------------------------------------------------");
        if (!lagrangeThere) {
            log("warn", "this file does not contain phase2 precalculated values. Please run: \n" +
                "   snarkjs \"powersoftau preparephase2\" to prepare this file to be used in the phase2 ceremony.");
        } else {
            for (const t of [2, 3, 4, 5]) {
                if (sec[t].lagThrow) throw new PtauRefusal(sec[t].lagThrow, { throws: true });
                if (!sec[t].ladder.every((v) => v)) { log("error", "Phase2 caclutation does not match with powers of tau"); return false; }
            }
        }
        log("info", "Powers of Tau Ok!");
        return true;
    } finally { rd.close(); }
}

module.exports = { verify, deviceOf, readContributions, firstChallengeHash, g2sp, PtauRefusal };
