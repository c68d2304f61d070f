// tests/js/concurrent_provers_gpu.js — GPU: the three fused provers of one process used AT THE SAME TIME (snarkjs_amd/js/plonk_native.js, fflonk_native.js,
// groth16_native.js behind js/device_queue.js). Each serialised only itself before, all of them on pipeline slot 0, so concurrent calls of different protocols
// collected each other's window sums. Every expected proof is the reference's own seeded proof (tests/golden/*.json: proof_sha256), never a serial run of this code:
// PLONK and FFLONK with the recorded blinding values, Groth16 with the recorded Fr.random draws handed to a stub `snarkjs` (as tests/js/native_gpu.js does).
//   1  three protocols at once: PLONK proveAsync + FFLONK proveAsync + two Groth16 prove calls (two, so that the pump submits and collects), all six start orders x 3 rounds
//   2  curves mixed: PLONK on BLS12-381 with Groth16 on BN254, and the reverse
//   3  sync in the middle: Groth16 proofs pending after one turn of the event loop, then the synchronous PLONK prove / proveMany and FFLONK prove: golden or the
//      library's busy-slot error, the pending proofs golden, nothing resolves to a wrong proof
//   3b a synchronous PLONK proveMany that fails in the middle: the reference's message, nothing leaked, both slots free afterwards
//   4  a verify batch of 256 proofs alongside a PLONK and a Groth16 proof
//   5  errors stay local: a truncated witness rejects its own promise only, with the reference's message
//   6  through registerAll(snarkjs, { fused: true }) where the reference's bundle is staged (oracle/_ref): fresh randomness, the reference's own verify
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/concurrent_provers_gpu.js
"use strict";
const fs = require("fs"), path = require("path"), crypto = require("crypto");
const ROOT = path.join(__dirname, "..", "..");
const JS = path.join(ROOT, "snarkjs_amd", "js");
const plonkN = require(path.join(JS, "plonk_native.js")), fflonkN = require(path.join(JS, "fflonk_native.js"));
const { makeProver } = require(path.join(JS, "groth16_native.js"));
const { pointToObject } = require(path.join(JS, "groth16_shards.js"));
const GOLD = path.join(ROOT, "tests", "golden");
const sha = (b) => crypto.createHash("sha256").update(b).digest("hex");
const hexb = (s) => new Uint8Array(Buffer.from(s, "hex"));
const rd = (p) => new Uint8Array(fs.readFileSync(p));
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }
const turn = () => new Promise((resolve) => setImmediate(resolve));
const settle = (ps) => Promise.all(ps.map((p) => p.then((v) => ({ v }), (e) => ({ e: e.message }))));
const BUSY = /pipeline slot \d holds work in flight/;

function fixture(tag) {
    const g = JSON.parse(fs.readFileSync(path.join(GOLD, tag + ".json")));
    return { tag, g, zkeyPath: path.join(GOLD, tag + ".zkey"), zkey: rd(path.join(GOLD, tag + ".zkey")), wtns: rd(path.join(GOLD, tag + ".wtns")),
             blind: g.blinding_mont ? g.blinding_mont.map(hexb) : null };
}
const golden = (fx, res) => !!res && !!res.proof && sha(JSON.stringify(res.proof)) === fx.g.proof_sha256 && JSON.stringify(res.publicSignals) === JSON.stringify(fx.g.publicSignals);
// a Groth16 witness one element short, with a consistent container: refused by the reference's length check (src/groth16_prove.js:45-47)
function shortGroth16(wtns) {
    const short = wtns.slice(0, wtns.length - 32), nBytes = wtns.length - 32;
    const dv = new DataView(short.buffer);
    let off = 12;
    for (let i = 0, k = dv.getUint32(8, true); i < k; i++) {
        const t = dv.getUint32(off, true), ln = Number(dv.getBigUint64(off + 4, true));
        if (t === 2) { dv.setBigUint64(off + 4, BigInt(nBytes - off - 12), true); break; }
        off += 12 + ln;
    }
    return short;
}

(async () => {
    const P = {}, F = {}, G = {};
    for (const tag of ["plonk_bn128_small", "plonk_bn128_n2048", "plonk_bls12381_small"]) { P[tag] = fixture(tag); P[tag].key = new plonkN.PlonkKey(P[tag].zkey); }
    for (const tag of ["fflonk_bn128_small", "fflonk_bn128_n256"]) { F[tag] = fixture(tag); F[tag].key = new fflonkN.FflonkKey(F[tag].zkey); }
    for (const [tag, cid, name] of [["groth16_bn128_n1024", 0, "bn128"], ["groth16_bls12381_n1024", 1, "bls12381"]]) {
        const fx = G[tag] = fixture(tag);
        // every draw of this prover is the recorded (r, s) pair in turn: whichever call draws first, each proof gets the reference's two values
        let k = 0;
        const curve = { name, Fr: { random: () => hexb(k++ % 2 === 0 ? fx.g.r_mont : fx.g.s_mont) }, G1: { toObject: (b) => pointToObject(cid, 1, b) }, G2: { toObject: (b) => pointToObject(cid, 2, b) } };
        fx.prover = makeProver({ curves: { getCurveFromName: async () => curve } });
        fx.prove = () => fx.prover.prove(fx.zkey, fx.wtns);
        check(`${tag}: a first proof alone (key load) is golden`, golden(fx, await fx.prove()));
    }
    const plonk = (fx, wtns) => plonkN.proveAsync(fx.key, wtns || fx.wtns, fx.blind);
    const fflonk = (fx, wtns) => fflonkN.proveAsync(fx.key, wtns || fx.wtns, fx.blind);
    const pTags = Object.keys(P), fTags = Object.keys(F), gTags = Object.keys(G);

    // ---- 1: three protocols at once, every start order
    const orders = [["p", "f", "g"], ["p", "g", "f"], ["f", "p", "g"], ["f", "g", "p"], ["g", "p", "f"], ["g", "f", "p"]];
    let n = 0;
    for (const order of orders) for (let round = 0; round < 3; round++, n++) {
        const p = P[pTags[n % 3]], f = F[fTags[n % 2]], g = G[gTags[n % 2]];
        const started = [];
        for (const who of order) {
            if (who === "p") started.push(["plonk " + p.tag, p, plonk(p)]);
            if (who === "f") started.push(["fflonk " + f.tag, f, fflonk(f)]);
            if (who === "g") { started.push(["groth16 " + g.tag, g, g.prove()]); started.push(["groth16 " + g.tag + " (second)", g, g.prove()]); }
        }
        const out = await settle(started.map((x) => x[2]));
        const bad = [];
        started.forEach((x, i) => { if (!golden(x[1], out[i].v)) bad.push(x[0] + ": " + (out[i].e || "not the golden proof")); });
        check(`three protocols at once, start order ${order.join("")}, round ${round}: ${started.map((x) => x[0]).join(", ")}`, bad.length === 0, JSON.stringify(bad));
    }

    // ---- 2: curves mixed
    for (const [pt, gt] of [["plonk_bls12381_small", "groth16_bn128_n1024"], ["plonk_bn128_n2048", "groth16_bls12381_n1024"]]) {
        const out = await settle([G[gt].prove(), plonk(P[pt]), G[gt].prove(), plonk(P[pt]), G[gt].prove()]);
        check(`curves mixed: ${pt} with ${gt}, interleaved in arrival order`, [G[gt], P[pt], G[gt], P[pt], G[gt]].every((fx, i) => golden(fx, out[i].v)), JSON.stringify(out.map((x) => x.e || "")));
    }

    // ---- 3: a synchronous prover in the middle of pending Groth16 proofs
    const syncCalls = [["plonk prove", () => [plonkN.prove(P.plonk_bn128_n2048.key, P.plonk_bn128_n2048.wtns, P.plonk_bn128_n2048.blind)], P.plonk_bn128_n2048],
                       ["plonk proveMany", () => plonkN.proveMany(P.plonk_bn128_small.key, [P.plonk_bn128_small.wtns, P.plonk_bn128_small.wtns, P.plonk_bn128_small.wtns],
                                                                  [P.plonk_bn128_small.blind, P.plonk_bn128_small.blind, P.plonk_bn128_small.blind]), P.plonk_bn128_small],
                       ["fflonk prove", () => [fflonkN.prove(F.fflonk_bn128_n256.key, F.fflonk_bn128_n256.wtns, F.fflonk_bn128_n256.blind)], F.fflonk_bn128_n256]];
    for (const [name, run, fx] of syncCalls) for (const gt of gTags) for (let turns = 1; turns <= 2; turns++) {
        const g = G[gt], pending = [g.prove(), g.prove(), g.prove()];
        for (let i = 0; i < turns; i++) await turn();
        let res = null, msg = "";
        try { res = run(); } catch (e) { msg = e instanceof Error ? e.message : "not an Error: " + e; }
        const out = await settle(pending);
        const how = res ? "returned" : "threw: " + msg;
        check(`sync ${name} after ${turns} turn(s) with three ${gt} proofs pending: golden or the busy-slot error (${how})`, res ? res.every((r) => golden(fx, r)) : BUSY.test(msg));
        check(`... and the pending ${gt} proofs are golden`, out.every((x) => golden(g, x.v)), JSON.stringify(out.map((x) => x.e || "")));
        let after = null;
        try { after = run(); } catch (e) { msg = e.message; }
        check(`... and the same sync ${name} with nothing pending is golden`, !!after && after.every((r) => golden(fx, r)), msg);
    }

    // ---- 3b: proveMany gives up in the middle (a witness that fails behind a commitment round, the other proof stopped between enqueue and collect): the reference's
    // message, every device buffer the call allocated is freed again, and neither slot stays busy
    for (const tag of ["plonk_bn128_small", "plonk_bls12381_small"]) {
        const p = P[tag], g = G.groth16_bn128_n1024, addon = plonkN._internals.addon, realCall = addon.call;
        const bad = p.wtns.slice(); bad[bad.length - 32] ^= 1;
        let allocs = 0, frees = 0, msg = "";
        addon.call = function (name) { if (name === "zkmi_dev_alloc") allocs++; else if (name === "zkmi_dev_free") frees++; return realCall.apply(this, arguments); };
        try { plonkN.proveMany(p.key, [p.wtns, bad, p.wtns, p.wtns], [p.blind, p.blind, p.blind, p.blind]); } catch (e) { msg = e.message; } finally { addon.call = realCall; }
        check(`${tag}: proveMany with a bad witness in the middle fails with the reference's message (${msg})`, /Copy constraints does not match|not divisible|not well calculated/.test(msg));
        check(`${tag}: ... and frees every device buffer it allocated (${allocs} allocated, ${frees} freed)`, allocs > 0 && allocs === frees);
        const out = await settle([g.prove(), g.prove(), g.prove()]);          // submit / collect in both slots
        check(`${tag}: ... Groth16 proofs in both slots afterwards are golden`, out.every((x) => golden(g, x.v)), JSON.stringify(out.map((x) => x.e || "")));
        let many = null;
        try { many = plonkN.proveMany(p.key, [p.wtns, p.wtns, p.wtns], [p.blind, p.blind, p.blind]); } catch (e) { msg = e.message; }
        check(`${tag}: ... and a PLONK proveMany over both slots is golden`, !!many && many.length === 3 && many.every((r) => golden(p, r)), msg);
    }

    // ---- 4: a verify batch alongside
    {
        const { VerifyingKey } = require(path.join(JS, "plonk_verify_native.js"));
        const p = P.plonk_bn128_n2048, g = G.groth16_bn128_n1024;
        const vk = new VerifyingKey(p.g.vk, { device: 0 });
        const pubs = [], proofs = [];
        for (let i = 0; i < 256; i++) { pubs.push(p.g.publicSignals); proofs.push(p.g.proof); }
        const [verdicts, pr, gr] = await Promise.all([vk.verifyMany(pubs, proofs), plonk(p), g.prove()]);
        check("256 golden PLONK proofs verified alongside a PLONK and a Groth16 proof: every verdict true, both proofs golden",
              verdicts.length === 256 && verdicts.every((v) => v === true) && golden(p, pr) && golden(g, gr));
        vk.release();
    }

    // ---- 5: errors stay local
    {
        const p = P.plonk_bn128_small, f = F.fflonk_bn128_small, g = G.groth16_bn128_n1024;
        const cut = (w) => w.subarray(0, w.length - 32);
        const sets = [["plonk", () => [plonk(p, cut(p.wtns)), fflonk(f), g.prove(), g.prove()], 0],
                      ["fflonk", () => [g.prove(), fflonk(f, cut(f.wtns)), plonk(p), g.prove()], 1],
                      ["groth16", () => [fflonk(f), g.prove(), g.prover.prove(g.zkey, shortGroth16(g.wtns)), plonk(p), g.prove()], 2]];
        for (const [who, start, badAt] of sets) {
            const fxs = who === "plonk" ? [p, f, g, g] : who === "fflonk" ? [g, f, p, g] : [f, g, g, p, g];
            const out = await settle(start());
            check(`a truncated ${who} witness rejects only its own promise, with the reference's message: ${out[badAt].e}`,
                  out.every((x, i) => (i === badAt ? /Invalid witness length/.test(x.e || "") : golden(fxs[i], x.v))), JSON.stringify(out.map((x) => x.e || "")));
        }
        check("a serial proof of each protocol afterwards is golden", golden(p, await plonk(p)) && golden(f, await fflonk(f)) && golden(g, await g.prove()));
    }

    for (const fx of Object.values(P).concat(Object.values(F))) fx.key.release();
    for (const fx of Object.values(G)) await fx.prover.release();

    // ---- 6: behind snarkjs's own entry points
    if (!fs.existsSync(path.join(ROOT, "oracle", "_ref", "build", "snarkjs.min.js"))) {
        console.log("NOT CHECKED ON THIS BOX: concurrent snarkjs.groth16 / plonk / fflonk .prove through registerAll(snarkjs, { fused: true }) needs the reference's bundle in " +
                    "oracle/_ref (`make -C oracle _ref` stages it where the reference is present)");
    } else {
        process.env.NTHREADS = process.env.NTHREADS || "8";
        process.env.ORACLE_UNSEEDED = "1";                  // fresh randomness
        const snarkjs = require(path.join(ROOT, "oracle", "ref_shim.js"));
        const { registerAll, uninstallFused, unregister } = require(path.join(JS, "register.js"));
        await registerAll(snarkjs, { fused: true });
        const g = G.groth16_bn128_n1024, p = P.plonk_bn128_n2048, f = F.fflonk_bn128_n256;
        for (let round = 0; round < 3; round++) {
            const calls = [["groth16", g, snarkjs.groth16.prove(g.zkeyPath, g.wtns)], ["plonk", p, snarkjs.plonk.prove(p.zkeyPath, p.wtns)], ["fflonk", f, snarkjs.fflonk.prove(f.zkeyPath, f.wtns)],
                           ["groth16", g, snarkjs.groth16.prove(g.zkeyPath, g.wtns)]];
            if (round % 2) calls.reverse();
            const out = await settle(calls.map((x) => x[2]));
            for (let i = 0; i < calls.length; i++) {
                const [proto, fx] = calls[i], r = out[i].v;
                const ok = !!r && JSON.stringify(r.publicSignals) === JSON.stringify(fx.g.publicSignals) && sha(JSON.stringify(r.proof)) !== fx.g.proof_sha256 &&
                           (await snarkjs[proto].verify(fx.g.vk, r.publicSignals, r.proof)) === true;
                check(`round ${round}: concurrent snarkjs.${proto}.prove (fused, fresh randomness) is accepted by the reference's verify`, ok, out[i].e || "");
            }
        }
        await uninstallFused(snarkjs);
        for (const name of ["bn128", "bls12381"]) unregister(await snarkjs.curves.getCurveFromName(name));
    }
    console.log(fails ? `${fails} FAILED` : "ALL OK");
    process.exit(fails ? 1 : 0);
})().catch((e) => { console.log("ERROR", e && e.stack || e); process.exit(2); });
