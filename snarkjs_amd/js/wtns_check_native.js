// snarkjs_amd/js/wtns_check_native.js — snarkjs.wtns.check (src/wtns_check.js) through the addon: async check(r1cs, wtns, logger, { addon | dev }) -> true | false,
// with the reference's info / warn lines in its order on `logger`. The twin of snarkjs_amd/wtns_check.py (DESIGN.md 22). The reference evaluates three sparse
// dot products per constraint in one JavaScript loop; here the constraints become a resident layout (addon.r1csLoad) and the witness one call (addon.r1csCheck)
// that returns the first failing constraint.
//
// Everything is read and looked over BEFORE a line is logged or the device is touched; whatever the reference would refuse, or would read beyond a buffer for,
// is handed to the saved reference function (WtnsRefusal.handOver): a file that is not well-formed, a missing or repeated section, a prime of neither curve, a
// witness of another prime, a constraint section that ends early, a signal id at or beyond the witness's length, a witness beyond one 2^30-byte buffer, inputs
// the readers do not take. The failing branch calls a LIVE logger.warn, so a bad witness with no logger throws what the reference throws.
// options.dev replaces the device calls (tests/js/wtns_check_cpu.js: a plain JS evaluation in their place); they may return promises.
"use strict";
const { readerOf, sectionTable } = require("./groth16_native.js");

const PRIMES = [
    { name: "bn128", id: 0, r: 21888242871839275222246405745257275088548364400416034343698204186575808495617n },
    { name: "bls12381", id: 1, r: 52435875175126190479447740508185965837690552500527637822603658699938581184513n },
];
const BIG_PAGE = 1 << 30, NONE = 0xFFFFFFFF, PROGRESS_EVERY = 500000;

// a call left to the reference itself
class WtnsRefusal extends Error {
    constructor(message, flags) { super(message); Object.assign(this, flags || {}); }
}
const handOver = (why) => new WtnsRefusal(why, { handOver: true });
const leBig = (b) => { let v = 0n; for (let i = b.length - 1; i >= 0; i--) v = (v << 8n) | BigInt(b[i]); return v; };

// the i of the reference's `··· processing r1cs constraints i/n` lines: every positive multiple of 500000 its loop reaches
function progressIndices(nConstraints, firstBad) {
    const stop = firstBad === null ? nConstraints - 1 : firstBad, out = [];
    for (let i = PROGRESS_EVERY; i <= stop; i += PROGRESS_EVERY) out.push(i);
    return out;
}

let nextKey = 0x57c000000000;
function deviceOf(addon) {
    return {
        load(cv, constraints, nConstraints, nVars) { const key = ++nextKey; addon.r1csLoad(cv.id, constraints, nConstraints, nVars, key); return key; },
        check(key, witnesses, nWitnesses) {
            const raw = addon.r1csCheck(key, witnesses, nWitnesses), dv = new DataView(raw.buffer, raw.byteOffset, raw.byteLength);
            return Array.from({ length: nWitnesses }, (_, k) => dv.getUint32(4 * k, true));
        },
        release(key) { addon.call("zkmi_r1cs_release", key); },
    };
}

function uniqueSection(tab, id) {
    if (!tab[id] || tab[id].length != 1) throw handOver(`section ${id} missing or repeated`);
    return tab[id][0];
}
// section 2 of the r1cs as pages of at most 2^30 bytes, after a pass over its term counts and signal ids: the offsets must stay inside the section and the ids
// below `nValues`, the number of values the witness holds (the reference indexes the witness by them and never looks at nVars)
function constraintPages(rd, s, nConstraints, nValues) {
    const pages = [];
    for (let o = 0; o < s.len; o += BIG_PAGE) pages.push(rd.read(s.pos + o, Math.min(BIG_PAGE, s.len - o)));
    let p = 0, off = 0;
    const settle = () => { while (p < pages.length && off == pages[p].length) { p++; off = 0; } return p < pages.length; };
    const u32 = () => {
        let v = 0;
        for (let i = 0; i < 4; i++) { if (!settle()) throw handOver("the constraint section ends early"); v += pages[p][off++] * 2 ** (8 * i); }
        return v;
    };
    const skip = (n) => { while (n) { if (!settle()) throw handOver("the constraint section ends early"); const k = Math.min(n, pages[p].length - off); off += k; n -= k; } };
    for (let l = 0; l < 3 * nConstraints; l++)
        for (let t = 0, n = u32(); t < n; t++) { if (u32() >= nValues) throw handOver("a signal id beyond the witness"); skip(32); }
    return pages.length == 1 ? pages[0] : (pages.length ? pages : new Uint8Array(0));
}

// Everything wtns.check reads, or a WtnsRefusal with handOver
function readInputs(r1csSrc, wtnsSrc) {
    let rd1 = null, rd2 = null;
    try {
        rd1 = readerOf(r1csSrc); rd2 = readerOf(wtnsSrc);
        const t1 = sectionTable(rd1, "r1cs"), t2 = sectionTable(rd2, "wtns");
        const v1 = rd1.read(4, 4), v2 = rd2.read(4, 4);
        if (new DataView(v1.buffer, v1.byteOffset, 4).getUint32(0, true) > 1 || new DataView(v2.buffer, v2.byteOffset, 4).getUint32(0, true) > 2) throw handOver("version");
        for (const [rd, tab] of [[rd1, t1], [rd2, t2]]) for (const id of Object.keys(tab)) for (const s of tab[id]) if (s.pos + s.len > rd.size) throw handOver("a section beyond the end of the file");
        const h1 = uniqueSection(t1, 1), c2 = uniqueSection(t1, 2), h2 = uniqueSection(t2, 1), w2 = uniqueSection(t2, 2);
        if (h1.len != 4 + 32 + 28 || h2.len != 4 + 32 + 4) throw handOver("header size");
        const a = Uint8Array.from(rd1.read(h1.pos, h1.len)), b = Uint8Array.from(rd2.read(h2.pos, h2.len));
        const av = new DataView(a.buffer), bv = new DataView(b.buffer);
        if (av.getUint32(0, true) != 32 || bv.getUint32(0, true) != 32) throw handOver("field size");
        const prime = leBig(a.subarray(4, 36)), cv = PRIMES.find((c) => c.r === prime);
        if (!cv || leBig(b.subarray(4, 36)) !== prime) throw handOver("prime");
        const head = { nVars: av.getUint32(36, true), nOutputs: av.getUint32(40, true), nPubInputs: av.getUint32(44, true), nPrvInputs: av.getUint32(48, true),
                       nLabels: Number(av.getBigUint64(52, true)), nConstraints: av.getUint32(60, true), useCustomGates: !!(t1[4] && t1[5]) };
        if (w2.len >= BIG_PAGE || w2.len % 32) throw handOver("witness section");
        const witness = Uint8Array.from(rd2.read(w2.pos, w2.len));
        const constraints = constraintPages(rd1, c2, head.nConstraints, witness.length / 32);
        return { cv, head, witness, constraints };
    } catch (e) {
        if (e instanceof WtnsRefusal) throw e;
        throw handOver(e.message);                          // whatever the readers could not take: the reference says it its own way
    } finally {
        if (rd1) rd1.close();
        if (rd2) rd2.close();
    }
}

async function check(r1csSrc, wtnsSrc, logger, options) {
    options = options || {};
    const { cv, head, witness, constraints } = readInputs(r1csSrc, wtnsSrc);
    const dev = options.dev || deviceOf(options.addon);
    if (logger) {
        for (const line of ["WITNESS CHECKING STARTED", "> Reading r1cs file", "> Reading witness file", "----------------------------", "  WITNESS CHECK", `  Curve:          ${cv.name}`,
                            `  Vars (wires):   ${head.nVars}`, `  Outputs:        ${head.nOutputs}`, `  Public Inputs:  ${head.nPubInputs}`, `  Private Inputs: ${head.nPrvInputs}`,
                            `  Labels:         ${head.nLabels}`, `  Constraints:    ${head.nConstraints}`, `  Custom Gates:   ${head.useCustomGates}`, "----------------------------",
                            "> Checking witness correctness"]) logger.info(line);
    }
    const key = await dev.load(cv, constraints, head.nConstraints, witness.length / 32);
    let first;
    try { first = (await dev.check(key, witness, 1))[0]; } finally { await dev.release(key); }
    const firstBad = first === NONE ? null : first;
    if (logger) for (const i of progressIndices(head.nConstraints, firstBad)) logger.info(`··· processing r1cs constraints ${i}/${head.nConstraints}`);
    if (firstBad !== null) {
        logger.warn("··· aborting checking process at constraint " + firstBad);        // no logger: the reference's TypeError
        logger.warn("WITNESS IS NOT CORRECT");
        logger.warn("WITNESS CHECKING FINISHED UNSUCCESSFULLY");
        return false;
    }
    if (logger) { logger.info("WITNESS IS CORRECT"); logger.info("WITNESS CHECKING FINISHED SUCCESSFULLY"); }
    return true;
}

module.exports = { check, readInputs, deviceOf, progressIndices, WtnsRefusal, PRIMES, NONE };
