// tests/js/wtns_check_cpu.js — js/wtns_check_native.js without a device (tests/test_node_wtns_check.py): behind installWtnsCheck(snarkjs, { dev }) (register.js: what
// registerAll(snarkjs, { wtnsCheck: true, dev }) installs) with a device written in plain JS (BigInt, one object per combination), every case of tests/golden/wtns_check_golden.json runs through the replacement and
// through the reference's LIVE function under a recording logger, on the same bytes:
//   1  the reference's live answer is the recorded one (cases where it reads beyond a buffer excepted: its answer there comes from stale memory)
//   2  the replacement returns or throws the same, with the same lines at the same levels, with a logger and without one
//   3  every hand-off case reaches the saved function before any device call and before any line of the replacement's own
//   4  from paths and fastfile descriptors as from bytes; unregister gives the reference's function back
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/wtns_check_cpu.js
"use strict";
const fs = require("fs"), os = require("os"), path = require("path");
const ROOT = path.join(__dirname, "..", "..");
process.env.NTHREADS = process.env.NTHREADS || "4";
const snarkjs = require(path.join(ROOT, "oracle", "ref_shim.js"));
const { installWtnsCheck, unregister } = require(path.join(ROOT, "snarkjs_amd", "js", "register.js"));
const wtnsN = require(path.join(ROOT, "snarkjs_amd", "js", "wtns_check_native.js"));
const GOLD = path.join(ROOT, "tests", "golden");
const CASES = JSON.parse(fs.readFileSync(path.join(GOLD, "wtns_check_golden.json"))).cases;
const G = (f) => new Uint8Array(fs.readFileSync(path.join(GOLD, f)));
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }

function recorder() {
    const lines = [], push = (level) => (text) => lines.push([level, text]);
    return { lines, logger: { debug: push("debug"), log: push("log"), info: push("info"), warn: push("warn"), error: push("error") } };
}
async function capture(f, withLogger) {
    const rec = recorder();
    try { return { returns: await f(withLogger ? rec.logger : undefined), lines: rec.lines }; } catch (e) { return { throws: e.message, lines: rec.lines }; }
}
const sameLines = (a, b) => JSON.stringify(a) === JSON.stringify(b);

// the device calls in plain JS: the reference's loop on BigInt
const calls = [];
const le = (b, o) => { let v = 0n; for (let i = 31; i >= 0; i--) v = (v << 8n) | BigInt(b[o + i]); return v; };
const plainDev = {
    loaded: new Map(), next: 1,
    load(cv, constraints, nConstraints, nVars) {
        calls.push("load");
        const sec = Array.isArray(constraints) ? Buffer.concat(constraints) : constraints;
        this.loaded.set(this.next, { r: cv.r, sec, nConstraints, nVars });
        return this.next++;
    },
    check(key, witnesses, n) {
        calls.push("check");
        const { r, sec, nConstraints, nVars } = this.loaded.get(key), dv = new DataView(sec.buffer, sec.byteOffset, sec.byteLength), out = [];
        for (let k = 0; k < n; k++) {
            let pos = 0, bad = wtnsN.NONE;
            const lc = () => { const m = {}, cnt = dv.getUint32(pos, true); pos += 4; for (let t = 0; t < cnt; t++, pos += 36) m[dv.getUint32(pos, true)] = le(sec, pos + 4) % r; return m; };
            const ev = (m) => Object.keys(m).reduce((acc, s) => (acc + le(witnesses, (k * nVars + Number(s)) * 32) % r * m[s]) % r, 0n);
            for (let i = 0; i < nConstraints && bad === wtnsN.NONE; i++) { const a = ev(lc()), b = ev(lc()), c = ev(lc()); if ((a * b - c) % r !== 0n) bad = i; }
            out.push(bad);
        }
        return out;
    },
    release(key) { calls.push("release"); this.loaded.delete(key); },
};

async function main() {
    const orig = snarkjs.wtns.check;
    let reached = 0;
    const counting = async function (...a) { reached++; return orig.apply(this, a); };
    snarkjs.wtns = Object.freeze(Object.assign({}, snarkjs.wtns, { check: counting }));          // the "reference function" the replacement saves
    installWtnsCheck(snarkjs, { dev: plainDev });               // what registerAll(snarkjs, { wtnsCheck: true, dev }) does, without binding a device for the curves
    check("the install replaces wtns.check", snarkjs.wtns.check !== counting && snarkjs.wtns.check !== orig);
    const tmp = fs.mkdtempSync(path.join(os.tmpdir(), "wtns_check_"));
    try {
        for (const c of CASES) {
            const r1cs = G(c.r1cs), wtns = G(c.wtns);
            const handOff = c.readsPast || c.throws !== undefined;
            for (const withLogger of [true, false]) {
                const label = `${c.name}${withLogger ? "" : " (no logger)"}`, want = withLogger ? c : c.noLogger;
                const ref = await capture((lg) => orig(r1cs, wtns, lg), withLogger);
                if (!c.readsPast) check(`${label}: the reference's live answer is the recorded one`, ref.returns === want.returns && ref.throws === want.throws && (!withLogger || sameLines(ref.lines, c.lines)),
                                        JSON.stringify([ref.returns, ref.throws]));
                calls.length = 0; reached = 0;
                const got = await capture((lg) => snarkjs.wtns.check(r1cs, wtns, lg), withLogger);
                if (handOff) {
                    check(`${label}: handed over before any device work`, reached === 1 && calls.length === 0, JSON.stringify([reached, calls]));
                    if (c.throws !== undefined) check(`${label}: the reference's thrown message and lines`, got.throws === ref.throws && sameLines(got.lines, ref.lines), JSON.stringify([got.throws, ref.throws]));
                } else {
                    check(`${label}: the same verdict or thrown message`, got.returns === ref.returns && got.throws === ref.throws, JSON.stringify([got.returns, got.throws, ref.returns, ref.throws]));
                    check(`${label}: the same lines`, sameLines(got.lines, ref.lines), JSON.stringify(got.lines) + " / " + JSON.stringify(ref.lines));
                    check(`${label}: one load, one check, one release, nothing handed over`, reached === 0 && calls.join() === "load,check,release" && plainDev.loaded.size === 0, JSON.stringify([reached, calls]));
                }
            }
        }
        // other kinds of input
        const by = Object.fromEntries(CASES.map((c) => [c.name, c]));
        for (const name of ["bn128_bad_two", "bls12381_good"]) {
            const c = by[name], p1 = path.join(tmp, "c.r1cs"), p2 = path.join(tmp, "w.wtns");
            fs.writeFileSync(p1, G(c.r1cs)); fs.writeFileSync(p2, G(c.wtns));
            for (const [kind, a, b] of [["paths", p1, p2], ["file descriptors", { type: "file", fileName: p1 }, { type: "file", fileName: p2 }], ["mem descriptors", { type: "mem", data: G(c.r1cs) }, { type: "mem", data: G(c.wtns) }]]) {
                reached = 0;
                const got = await capture((lg) => snarkjs.wtns.check(a, b, lg), true);
                check(`${name}: from ${kind}`, got.returns === c.returns && sameLines(got.lines, c.lines) && reached === 0, JSON.stringify([got.returns, got.throws]));
            }
        }
        reached = 0;
        const missing = await capture((lg) => snarkjs.wtns.check(path.join(tmp, "nothing.r1cs"), path.join(tmp, "w.wtns"), lg), true);
        check("a file that is not there: handed over, the reference throws", reached === 1 && missing.throws !== undefined, JSON.stringify(missing));
        check("progressIndices", JSON.stringify([wtnsN.progressIndices(500000, null), wtnsN.progressIndices(500001, null), wtnsN.progressIndices(1500001, 1000000), wtnsN.progressIndices(1500001, 999999)]) ===
              JSON.stringify([[], [500000], [500000, 1000000], [500000]]));
        unregister(snarkjs);
        check("unregister gives the saved function back", snarkjs.wtns.check === counting);
    } finally {
        fs.rmSync ? fs.rmSync(tmp, { recursive: true, force: true }) : fs.rmdirSync(tmp, { recursive: true });
    }
    console.log(fails ? `${fails} FAILED` : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.error(e); process.exit(1); });
