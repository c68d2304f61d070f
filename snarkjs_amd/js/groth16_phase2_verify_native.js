// snarkjs_amd/js/groth16_phase2_verify_native.js — snarkjs.zKey.verifyFromInit (src/zkey_verify_frominit.js) and zKey.verifyFromR1cs
// (src/zkey_verify_fromr1cs.js) through the addon: async verifyFromInit(init, ptau, zkey, { log, random64 }) -> true | false, with log(level, text) receiving the
// reference's lines, levels ("log" for what it prints with console.log) and order. The twin of snarkjs_amd/groth16_phase2_verify.py. Everything on curve
// points is one of three addon calls (include/zkmi.h, DESIGN.md 17): sameRatioBatch for the 2c + 1 checks of a key with c contributions in one launch and
// one for L and H together, phase2SectionRatio and phase2HRatio for the two sums of the L and of the H check. random64: bytes 0 - 31 are the L seed and
// bytes 32 - 63 the H seed, each as eight big-endian words. options.dev replaces the three calls, which may
// return promises (tests/js/phase2_verify_cpu.js: the reference's own curve in their place).
"use strict";
const crypto = require("crypto"), path = require("path");
const { readerOf, sectionTable } = require("./groth16_native.js");
const { Phase2Refusal, parseMpcParams, seedFromBeacon, hashPubKey, lemToUHost, leToBig, MAX_SECTION } = require("./groth16_phase2_native.js");
const setupN = require("./groth16_setup_native.js");

const CHUNK = 1 << 20;                 // MAX_CHUNK_SIZE of the reference's loops: one debug line per chunk

// misc.formatHash
function formatHash(b, title) {
    const a = Buffer.from(b.buffer, b.byteOffset, b.byteLength), rows = [];
    for (let i = 0; i < 4; i++) {
        const w = [];
        for (let j = 0; j < 4; j++) w.push(a.readUInt32BE(i * 16 + j * 4).toString(16).padStart(8, "0"));
        rows.push("\t\t" + w.join(" "));
    }
    return (title ? title + "\n" : "") + rows.join("\n");
}
const same = (a, b) => a.byteLength == b.byteLength && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;
// the eight big-endian words of 32 bytes, as the bytes of a Uint32Array (what the addon takes for a seed)
function seedBytes(b32) {
    const w = new Uint32Array(8), b = Buffer.from(b32.buffer, b32.byteOffset, 32);
    for (let i = 0; i < 8; i++) w[i] = b.readUInt32BE(4 * i);
    return new Uint8Array(w.buffer);
}

function deviceOf(addon) {
    const affine = (cv, jac) => { const out = new Uint8Array(2 * cv.n8q); addon.call("zkmi_to_affine", cv.id, 1, Uint8Array.from(jac), out); return out; };
    const pair = (cv, r) => [affine(cv, r.subarray(0, 3 * cv.n8q)), affine(cv, r.subarray(3 * cv.n8q))];
    return {
        sameRatioBatch(cv, checks) {
            if (!checks.length) return [];
            const cols = [0, 1, 2, 3].map((k) => new Uint8Array(Buffer.concat(checks.map((c) => Buffer.from(c[k])))));
            return Array.from(addon.sameRatioBatch(cv.id, cols[0], cols[1], cols[2], cols[3], checks.length), (v) => v === 1);
        },
        sectionRatio: (cv, a, b, n, seed32) => pair(cv, addon.phase2SectionRatio(cv.id, a, b, n, seedBytes(seed32))),
        hRatio: (cv, tau, h, power, seed32) => pair(cv, addon.phase2HRatio(cv.id, tau, h, power, seedBytes(seed32))),
        keyFromSeed(cv, seed) {
            const prv = new Uint8Array(32), s = new Uint8Array(2 * cv.n8q), sx = new Uint8Array(2 * cv.n8q);
            addon.call("zkmi_phase2_key_from_seed", cv.id, seed, prv, s, sx);
            return { g1_s: s, g1_sx: sx };
        },
        hashToG2(cv, transcript) { const out = new Uint8Array(4 * cv.n8q); addon.call("zkmi_phase2_hash_to_g2", cv.id, Uint8Array.from(transcript), out); return out; },
    };
}

// section table, curve record and the fields of section 2; `notGroth16`: the reference's message for another protocol. A section beyond one buffer hands over.
function openKey(rd, notGroth16) {
    const tab = sectionTable(rd, "zkey");
    const protocol = rd.read(tab[1][0].pos, 4);
    if (new DataView(protocol.buffer, protocol.byteOffset, 4).getUint32(0, true) != 1) throw new Phase2Refusal(notGroth16, { throws: true });
    for (const t of Object.keys(tab)) if (tab[t][0].len > MAX_SECTION) throw new Phase2Refusal("a section larger than one buffer", { handOver: true });
    const sec2 = rd.read(tab[2][0].pos, tab[2][0].len), dv = new DataView(sec2.buffer, sec2.byteOffset, sec2.byteLength);
    const n8q = dv.getUint32(0, true), q = leToBig(sec2.subarray(4, 4 + n8q)), cv = setupN.CURVES.find((c) => c.q === q);
    if (!cv) throw new Phase2Refusal(`Curve not supported: ${q}`, { throws: true });
    const n8r = dv.getUint32(4 + n8q, true);
    let o = 8 + n8q + n8r;
    const key = { n8q, n8r, q: sec2.subarray(4, 4 + n8q), r: sec2.subarray(8 + n8q, 8 + n8q + n8r), nVars: dv.getUint32(o, true), nPublic: dv.getUint32(o + 4, true), domainSize: dv.getUint32(o + 8, true) };
    o += 12;
    for (const [k, sz] of [["alpha1", 2 * n8q], ["beta1", 2 * n8q], ["beta2", 4 * n8q], ["gamma2", 4 * n8q], ["delta1", 2 * n8q], ["delta2", 4 * n8q]]) { key[k] = sec2.subarray(o, o + sz); o += sz; }
    return { tab, cv, key };
}
const section = (rd, tab, t) => rd.read(tab[t][0].pos, tab[t][0].len);
// an input the readers here do not take (a fastfile descriptor of another kind, { type: "bigMem" }) goes to the reference
function reader(src) { try { return readerOf(src); } catch (e) { throw new Phase2Refusal(e.message, { handOver: true }); } }

async function verifyFromInit(initSrc, ptauSrc, zkeySrc, options) {
    options = options || {};
    const log = options.log || (() => {});
    const dev = options.dev || deviceOf(options.addon || require(path.join(__dirname, "..", "napi", "zkmi_napi.node")));
    const random64 = options.random64 || crypto.randomBytes(64);
    const rds = [];
    const open = (src) => { const r = reader(src); rds.push(r); return r; };
    try {
        const rd = open(zkeySrc), rdInit = open(initSrc), rdPtau = open(ptauSrc);
        const { tab, cv, key } = openKey(rd, "zkey file is not groth16");
        const s1 = 2 * cv.n8q, domain = key.domainSize, power = 31 - Math.clz32(domain);
        // what is left to the reference, found before a line is logged
        if (power >= cv.s || (2 * domain - 1) * s1 > MAX_SECTION) throw new Phase2Refusal("power >= Fr.s, or a tauG1 slice larger than one buffer", { handOver: true });
        const mpc = parseMpcParams(section(rd, tab, 10), cv);
        const { g1: g1Gen, g2: g2Gen } = setupN.generatorsLem(cv);

        // the contributions: everything but the pairings is host work, so the 2c + 1 same-ratio checks go to the device together; a check that an earlier
        // failure makes moot is left out of the launch
        const steps = [], checks = [], fed = [Buffer.from(mpc.csHash)];
        const blake = (bufs) => { const h = crypto.createHash("blake2b512"); for (const b of bufs) h.update(b); return h; };
        const pubKey = (c) => { const parts = [], h = { update: (b) => parts.push(Buffer.from(b)) }; hashPubKey(h, cv, c); return parts; };
        let curDelta = g1Gen, hostOk = true;
        for (let i = 0; i < mpc.contributions.length && hostOk; i++) {
            const c = mpc.contributions[i];
            const ours = blake(fed.concat([lemToUHost(cv, c.g1_s, 1), lemToUHost(cv, c.g1_sx, 1)])).digest();
            steps.push([`INVALID(${i}): Inconsistent transcript `, same(ours, c.transcript)]);
            if (!steps[steps.length - 1][1]) { hostOk = false; break; }
            const g2sp = dev.hashToG2(cv, c.transcript);
            steps.push([`INVALID(${i}): public key G1 and G2 do not have the same ration `, checks.length]);
            checks.push([c.g1_s, c.g1_sx, g2sp, c.g2_spx]);
            steps.push([`INVALID(${i}): deltaAfter does not fillow the public key `, checks.length]);
            checks.push([curDelta, c.deltaAfter, g2sp, c.g2_spx]);
            if (c.type == 1) {
                const k = dev.keyFromSeed(cv, seedFromBeacon(c.beaconHash, c.numIterationsExp));
                steps.push([`INVALID(${i}): Key of the beacon does not match. g1_s `, same(k.g1_s, c.g1_s)]);
                steps.push([`INVALID(${i}): Key of the beacon does not match. g1_sx `, same(k.g1_sx, c.g1_sx)]);
                if (!same(k.g1_s, c.g1_s) || !same(k.g1_sx, c.g1_sx)) { hostOk = false; break; }
            }
            const pk = pubKey(c);
            fed.push(...pk);
            c.contributionHash = new Uint8Array(blake(pk).digest());
            curDelta = c.deltaAfter;
        }
        let atDelta2 = -1;
        if (hostOk) { atDelta2 = checks.length; checks.push([g1Gen, curDelta, g2Gen, key.delta2]); }      // delta2 needs nothing of the init key: it rides along
        const verdicts = await dev.sameRatioBatch(cv, checks);
        for (const [msg, v] of steps) if (!(typeof v === "number" ? verdicts[v] : v)) { log("log", msg); return false; }

        // against the init key
        const { tab: tabInit, key: init } = openKey(rdInit, "zkeyinit file is not groth16");
        if (!same(init.q, key.q) || !same(init.r, key.r) || init.n8q != key.n8q || init.n8r != key.n8r) { log("error", "INVALID:  Different curves"); return false; }
        if (init.nVars != key.nVars || init.nPublic != key.nPublic || init.domainSize != key.domainSize) { log("error", "INVALID:  Different circuit parameters"); return false; }
        for (const k of ["alpha1", "beta1", "beta2", "gamma2"]) if (!same(key[k], init[k])) { log("error", `INVALID:  Invalid ${k}`); return false; }
        if (!same(key.delta1, curDelta)) { log("error", "INVALID:  Invalid delta1"); return false; }
        if (!verdicts[atDelta2]) { log("error", "INVALID:  Invalid delta2"); return false; }
        const mpcInit = parseMpcParams(section(rdInit, tabInit, 10), cv);
        if (!same(mpc.csHash, mpcInit.csHash)) { log("error", "INVALID:  Circuit does not match"); return false; }
        if (tab[8][0].len != s1 * (key.nVars - key.nPublic - 1)) { log("error", "INVALID:  Invalid L section size"); return false; }
        if (tab[9][0].len != s1 * domain) { log("error", "INVALID:  Invalid H section size"); return false; }
        for (const [t, msg] of [[3, "INVALID:  IC section is not identical"], [4, "Coeffs section is not identical"], [5, "A section is not identical"],
                                [6, "B1 section is not identical"], [7, "B2 section is not identical"]])
            if (!same(section(rd, tab, t), section(rdInit, tabInit, t))) { log("error", msg); return false; }

        // L and H. One lane's pairing is the time of a whole same-ratio launch, so the two checks share one: the sums of H are computed before the verdict on L is
        // known. The lines, and whatever the H side throws, still come in the reference's order: nothing of H is reported unless L has passed.
        const lInit = section(rdInit, tabInit, 8), nPoints = lInit.byteLength / s1, pending = [];
        if (nPoints) {
            const [r1, r2] = await dev.sectionRatio(cv, lInit, section(rd, tab, 8), nPoints, random64.subarray(0, 32));
            pending.push([r1, r2, key.delta2, init.delta2]);
        }
        let hError = null;
        try {
            const sp = sectionTable(rdPtau, "ptau");
            if (!sp[2] || sp[2][0].len < (2 * domain - 1) * s1) throw new Phase2Refusal("the ptau's tauG1 section holds fewer than 2 domainSize - 1 points", { throws: true });
            const [h1, h2] = await dev.hRatio(cv, rdPtau.read(sp[2][0].pos, (2 * domain - 1) * s1), section(rd, tab, 9), power, random64.subarray(32, 64));
            pending.push([h1, h2, key.delta2, init.delta2]);
        } catch (e) { hError = e; }
        const last = await dev.sameRatioBatch(cv, pending);
        for (let i = 0; i < nPoints; i += CHUNK) log("debug", `Same ratio check L section:  ${i}/${nPoints}`);
        if (nPoints && !last[0]) { log("error", "L section does not match"); return false; }
        if (hError) throw hError;
        for (const what of ["tau", "lagrange"]) for (let i = 0; i < domain; i += CHUNK) log("debug", `H Verification(${what}):  ${i}/${domain}`);
        if (!last[last.length - 1]) { log("error", "H section does not match"); return false; }

        log("info", formatHash(mpc.csHash, "Circuit Hash: "));
        for (let i = mpc.contributions.length - 1; i >= 0; i--) {
            const c = mpc.contributions[i];
            log("info", "-------------------------");
            log("info", formatHash(c.contributionHash, `contribution #${i + 1} ${c.name ? c.name : ""}:`));
            if (c.type == 1) {
                log("info", `Beacon generator: ${Buffer.from(c.beaconHash).toString("hex")}`);
                log("info", `Beacon iterations Exp: ${c.numIterationsExp}`);
            }
        }
        log("info", "-------------------------");
        log("info", "ZKey Ok!");
        return true;
    } finally { for (const r of rds) r.close(); }
}

// newZKey on the device in memory, then verifyFromInit. Of the lines the reference's newZKey logs on the way, the info lines are logged here as well; its
// debug progress lines are not. What the device newZKey refuses or hands over leaves the whole call to the reference.
async function verifyFromR1cs(r1csSrc, ptauSrc, zkeySrc, options) {
    options = options || {};
    const log = options.log || (() => {});
    const addon = options.addon || require(path.join(__dirname, "..", "napi", "zkmi_napi.node"));
    reader(zkeySrc).close();
    let made;
    try { made = setupN.newZKey(r1csSrc, ptauSrc, { addon }); } catch (e) {
        if (e instanceof setupN.SetupRefusal) throw new Phase2Refusal(e.message, { handOver: true });
        throw e;
    }
    for (const what of ["r1cs", "tauG1", "tauG2", "alphatauG1", "betatauG1"]) log("info", "Reading " + what);
    log("info", formatHash(made.csHash, "Circuit hash: "));
    return verifyFromInit(made.zkey, ptauSrc, zkeySrc, Object.assign({}, options, { addon }));
}

module.exports = { verifyFromInit, verifyFromR1cs, formatHash, deviceOf, Phase2Refusal };
