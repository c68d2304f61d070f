// tests/js/ptau_prepare_cpu.js — js/powersoftau_prepare_native.js without a device (tests/test_node_ptau_prepare.py): its parsing and the bytes it writes
// against the reference's LIVE powersOfTau.preparePhase2 and .convert, with the reference's own curve object (G.lagrangeEvaluations, power by power) in place of
// the device call. Per curve, on the same bytes:
//   1  the raw p6 ceremony, the p8 setup file and the raw p6 ceremony cut to power 4: preparePhase2 gives the same bytes; the first two are the committed
//      prepared files, the cut has header powers 4 / 4
//   2  convert of the prepared p6 file without its top block gives the prepared file; convert of the p8 file appends the top block a second time, live and here
//   3  a Groth16 zkey, a file without section 3, with section 2 twice, with section 4 one byte short: the driver hands the call over (PrepareRefusal.handOver);
//      through the installed functions such a call reaches the saved reference function: its thrown message, or for preparePhase2 of the short section 4, which the
//      reference reads without checking its end, its file
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/ptau_prepare_cpu.js
"use strict";
const path = require("path");
const L = require("./ptau_verify_lib.js");
process.env.NTHREADS = process.env.NTHREADS || "8";
const snarkjs = require(path.join(L.ROOT, "oracle", "ref_shim.js"));
const prepareN = require(path.join(L.ROOT, "snarkjs_amd", "js", "powersoftau_prepare_native.js"));
const setupN = require(path.join(L.ROOT, "snarkjs_amd", "js", "groth16_setup_native.js"));
const { installPtauPrepare, uninstallPtauPrepare } = require(path.join(L.ROOT, "snarkjs_amd", "js", "register.js"));
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }
const same = (a, b) => a.byteLength === b.byteLength && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;
const bytes = (m) => { const d = m.data; return (d instanceof Uint8Array) ? d : d.slice(0, d.byteLength); };

function refDevice(curve, cv) {
    const calls = [];
    return { calls,
        async lagrangeSection(_cv, group, tau, nTau, first, top, zeroLast) {
            const G = group == 1 ? curve.G1 : curve.G2, sg = 2 * group * cv.n8q, out = [];
            calls.push([group, nTau, first, top, zeroLast]);
            for (let p = first; p <= top; p++) {
                const n = 2 ** p, pts = new Uint8Array(n * sg);
                pts.set(tau.subarray(0, (p == top && zeroLast ? n - 1 : n) * sg));
                const r = await G.lagrangeEvaluations(pts, "affine", "affine");
                out.push(Buffer.from(r instanceof Uint8Array ? r : r.slice(0, r.byteLength)));
            }
            return new Uint8Array(Buffer.concat(out));
        } };
}
async function live(which, raw) {
    const out = { type: "mem" };
    await snarkjs.powersOfTau[which]({ type: "mem", data: raw }, out);
    return bytes(out);
}

async function main() {
    for (const name of ["bn128", "bls12381"]) {
        const curve = await snarkjs.curves.getCurveFromName(name), cv = setupN.CURVES.find((c) => c.name === name);
        const dev = refDevice(curve, cv), s1 = 2 * cv.n8q;
        const p6raw = L.G(`ptau_${name}_p6_c3b_raw.ptau`), p6 = L.G(`ptau_${name}_p6_c3b.ptau`), p8 = L.G(`setup_${name}_p8.ptau`);
        const cut = L.caseFile({ fixture: `ptau_${name}_p6_c3b_raw.ptau`, rule: "truncate4" }, cv.n8q);
        for (const [label, raw, want] of [["raw p6", p6raw, p6], ["p8", p8, p8], ["raw p6 cut to power 4", cut, null]]) {
            const ref = await live("preparePhase2", raw), got = await prepareN.preparePhase2(raw, { dev });
            check(`${name}: preparePhase2(${label}): the reference's bytes`, same(got, ref));
            if (want) check(`${name}: preparePhase2(${label}): the committed prepared file`, same(ref, want));
            else {
                const hv = L.split(got)[0][1];
                const dv = new DataView(hv.buffer, hv.byteOffset, hv.byteLength);
                check(`${name}: preparePhase2(${label}): header powers 4 / 4`, dv.getUint32(4 + cv.n8q, true) === 4 && dv.getUint32(8 + cv.n8q, true) === 4);
            }
        }
        check(`${name}: one call per section`, dev.calls.length === 12 && JSON.stringify(dev.calls.slice(0, 4)) === JSON.stringify([[1, 127, 0, 7, true], [2, 64, 0, 6, false], [1, 64, 0, 6, false], [1, 64, 0, 6, false]]));
        const noTop = L.join(p6, L.split(p6).map(([t, b]) => [t, t == 12 ? b.subarray(0, b.length - 128 * s1) : b]));
        const refA = await live("convert", noTop), gotA = await prepareN.convert(noTop, { dev });
        check(`${name}: convert(p6 without its top block): the reference's bytes, the prepared file`, same(gotA, refA) && same(refA, p6));
        const refB = await live("convert", p8), gotB = await prepareN.convert(p8, { dev });
        const doubled = L.join(p8, L.split(p8).map(([t, b]) => [t, t == 12 ? new Uint8Array(Buffer.concat([Buffer.from(b), Buffer.from(b.subarray(b.length - 512 * s1))])) : b]));
        check(`${name}: the live convert(p8) doubles the top block`, !same(refB, p8) && same(refB, doubled));
        check(`${name}: convert(p8): the reference's bytes`, same(gotB, refB));
        // files that are not well-formed: handed over by the driver; through the installed functions they reach the saved function and throw its message
        const secs = L.split(p6raw);
        const bad = [["a Groth16 zkey", L.G(name === "bn128" ? "groth16_bn128_n1024.zkey" : "groth16_bls12381_n1024.zkey")], ["no section 3", L.join(p6raw, secs.filter(([t]) => t != 3))],
                     ["section 2 twice", L.join(p6raw, secs.concat(secs.filter(([t]) => t == 2)))],
                     ["section 4 one byte short", L.join(p6raw, secs.map(([t, b]) => [t, t == 4 ? b.subarray(0, b.length - 1) : b]))]];
        const orig = { preparePhase2: snarkjs.powersOfTau.preparePhase2, convert: snarkjs.powersOfTau.convert };
        for (const [what, raw] of bad) for (const which of ["preparePhase2", "convert"]) {
            const n0 = dev.calls.length;
            const got = await L.capture(() => prepareN[which](raw, { dev }));
            check(`${name}: ${which}(${what}): handed over before any device work`, got.error !== undefined && dev.calls.length === n0, JSON.stringify(got.error));
            let handed = false;
            try { await prepareN[which](raw, { dev }); } catch (e) { handed = e instanceof prepareN.PrepareRefusal && e.handOver === true; }
            check(`${name}: ${which}(${what}): a PrepareRefusal with handOver`, handed);
            // the reference throws at all of these but one: preparePhase2 reads section 4 without checking its end, and writes a file
            const refOut = { type: "mem" }, instOut = { type: "mem" };
            const ref = await L.capture(() => orig[which]({ type: "mem", data: raw }, refOut));
            installPtauPrepare(snarkjs, { addon: { init() {}, ptauLagrangeSection() { throw new Error("the device was reached"); } } });
            const inst = await L.capture(() => snarkjs.powersOfTau[which]({ type: "mem", data: raw }, instOut));
            uninstallPtauPrepare(snarkjs);
            const throwsThere = !(which === "preparePhase2" && what === "section 4 one byte short");
            check(`${name}: ${which}(${what}): the saved function's ${throwsThere ? "message" : "file"}`,
                  throwsThere ? ref.error !== undefined && inst.error === ref.error : ref.error === undefined && inst.error === undefined && same(bytes(instOut), bytes(refOut)),
                  JSON.stringify([inst.error, ref.error]));
        }
        check(`${name}: uninstall restores the reference's functions`, snarkjs.powersOfTau.preparePhase2 === orig.preparePhase2 && snarkjs.powersOfTau.convert === orig.convert);
    }
    console.log(fails ? `${fails} FAILED` : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.error(e); process.exit(1); });
