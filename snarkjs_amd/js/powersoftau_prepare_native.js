// snarkjs_amd/js/powersoftau_prepare_native.js — snarkjs.powersOfTau.preparePhase2 and .convert (src/powersoftau_preparephase2.js, src/powersoftau_convert.js)
// through the addon: async preparePhase2(oldPtau, options) / convert(oldPtau, options) -> the new file's bytes (Uint8Array), byte for byte what the reference
// writes. The twin of snarkjs_amd/powersoftau_prepare.py (DESIGN.md 19). Everything on curve points is ptauLagrangeSection, once per section 2 - 5 from one
// upload: for p = first .. top the inverse group FFT of the first 2^p points (the reference makes one G.ifft per power, each with a re-read of the section).
// Section 12 goes to top = power + 1 with the last point of its top block taken as infinity; the new header states ceremonyPower = power (the reference calls
// writePTauHeader without one); convert copies the old sections 12 - 15 and appends the power + 1 block to section 12 whether it is there already or not.
// options.dev replaces the device call, which may return a promise (tests/js/ptau_prepare_cpu.js: the reference's own curve in its place). Handed to the saved
// reference function (PrepareRefusal.handOver): any file that is not well-formed (sections 1 - 7 once each with the sizes the header implies, for convert also
// 12 - 15 once each), power + 1 > Fr.s, a section beyond one 2^30-byte buffer, inputs the readers do not take. The reference's logger receives debug lines only;
// they are not reproduced.
"use strict";
const path = require("path");
const { readerOf, sectionTable } = require("./groth16_native.js");
const { leToBig, MAX_SECTION } = require("./groth16_phase2_native.js");
const setupN = require("./groth16_setup_native.js");

// a call left to the reference itself
class PrepareRefusal extends Error {
    constructor(message, flags) { super(message); Object.assign(this, flags || {}); }
}
const handOver = (message) => new PrepareRefusal(message, { handOver: true });

function deviceOf(addon) {
    return {
        // tau: Uint8Array of nTau points -> the blocks first .. top back to back, 2^(top + 1) - 2^first points
        lagrangeSection: (cv, group, tau, nTau, first, top, zeroLast) => addon.ptauLagrangeSection(cv.id, group, tau, nTau, first, top, zeroLast ? 1 : 0),
    };
}

// the sections and header of a well-formed file
function open(rd, withLagrange) {
    let tab;
    try { tab = sectionTable(rd, "ptau"); } catch (e) { throw handOver(e.message); }
    const version = (() => { const h = rd.read(0, 12); return new DataView(h.buffer, h.byteOffset, 12).getUint32(4, true); })();
    if (version > 1) throw handOver("Version not supported");
    const once = withLagrange ? [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15] : [1, 2, 3, 4, 5, 6, 7];
    let end = 12;
    for (const t of Object.keys(tab)) for (const s of tab[t]) {
        if (s.len > MAX_SECTION) throw handOver("a section larger than one buffer");
        end = Math.max(end, s.pos + s.len);
    }
    if (end > rd.size) throw handOver("a section beyond the end of the file");
    for (const t of once) if (!tab[t] || tab[t].length != 1) throw handOver(`section ${t} is not there exactly once`);
    const head = rd.read(tab[1][0].pos, tab[1][0].len);
    if (head.length < 4) throw handOver("Invalid PTau header size");
    const hv = new DataView(head.buffer, head.byteOffset, head.byteLength), n8 = hv.getUint32(0, true);
    if (head.length != 4 + n8 + 8) throw handOver("Invalid PTau header size");
    const q = leToBig(head.subarray(4, 4 + n8)), cv = setupN.CURVES.find((c) => c.q === q);
    if (!cv || cv.n8q != n8) throw handOver("Curve not supported");
    const power = hv.getUint32(4 + n8, true);
    if (power + 1 > cv.s) throw handOver("power + 1 > Fr.s");
    const s1 = 2 * n8, s2 = 4 * n8;
    for (const [t, size] of [[2, (2 * 2 ** power - 1) * s1], [3, 2 ** power * s2], [4, 2 ** power * s1], [5, 2 ** power * s1], [6, s2]])
        if (tab[t][0].len != size) throw handOver(`section ${t} has not the size the header implies`);
    return { tab, cv, power, head };
}

// writePTauHeader(fd, curve, power): the ceremony power defaults to the power
function headerOf(head, cv, power) {
    const out = Uint8Array.from(head), dv = new DataView(out.buffer);
    dv.setUint32(4 + cv.n8q, power, true); dv.setUint32(8 + cv.n8q, power, true);
    return out;
}

function fileOf(secs) {
    let size = 12;
    for (const [, parts] of secs) { size += 12; for (const p of parts) size += p.byteLength; }
    const out = new Uint8Array(size), dv = new DataView(out.buffer);
    out.set([0x70, 0x74, 0x61, 0x75], 0);                                                   // "ptau"
    dv.setUint32(4, 1, true); dv.setUint32(8, secs.length, true);
    let o = 12;
    for (const [typ, parts] of secs) {
        let len = 0;
        for (const p of parts) len += p.byteLength;
        dv.setUint32(o, typ, true); dv.setBigUint64(o + 4, BigInt(len), true);
        o += 12;
        for (const p of parts) { out.set(p, o); o += p.byteLength; }
    }
    return out;
}

const LADDERS = [[2, 12, 1, 1, true], [3, 13, 2, 0, false], [4, 14, 1, 0, false], [5, 15, 1, 0, false]];      // old section, new section, group, top - power, zero_last

async function run(src, options, isConvert) {
    options = options || {};
    const dev = options.dev || deviceOf(options.addon || require(path.join(__dirname, "..", "napi", "zkmi_napi.node")));
    let rd;
    try { rd = readerOf(src); } catch (e) { throw handOver(e.message); }
    try {
        const { tab, cv, power, head } = open(rd, isConvert);
        const body = (t) => rd.read(tab[t][0].pos, tab[t][0].len);
        const secs = [[1, [headerOf(head, cv, power)]]];
        for (let t = 2; t <= 7; t++) secs.push([t, [body(t)]]);
        if (isConvert) {
            const top = power + 1;
            secs.push([12, [body(12), await dev.lagrangeSection(cv, 1, secs[1][1][0], 2 ** top - 1, top, top, true)]]);
            for (const t of [13, 14, 15]) secs.push([t, [body(t)]]);
        } else {
            for (const [old, nu, group, up, zeroLast] of LADDERS) {
                const top = power + up, nTau = 2 ** top - (zeroLast ? 1 : 0), sg = 2 * group * cv.n8q;
                if ((2 * 2 ** top - 1) * sg > MAX_SECTION) throw handOver("a section larger than one buffer");
                secs.push([nu, [await dev.lagrangeSection(cv, group, secs[old - 1][1][0].subarray(0, nTau * sg), nTau, 0, top, zeroLast)]]);
            }
        }
        return fileOf(secs);
    } finally { rd.close(); }
}

const preparePhase2 = (src, options) => run(src, options, false);
const convert = (src, options) => run(src, options, true);

module.exports = { preparePhase2, convert, deviceOf, PrepareRefusal, open, headerOf, fileOf };
