// tests/js/fflonk_setup_gpu.js — snarkjs.fflonk.setup on the device through the real addon (tests/test_gpu_fflonk_setup.py).
//   1  registerAll(snarkjs) and { plonkSetup: true } leave snarkjs.fflonk.setup the reference's
//   2  registerAll(snarkjs, { fflonkSetup: true }): fflonk.setup on the edge fixture writes the golden key (path and fastfile mem target)
//   3  the reference's refusals are thrown with its words
//   4  a BLS12-381 ceremony reaches the original function: the same bytes as without the option
//   5  unregister(snarkjs) restores the reference's function, which still produces the same key
// Run:  node --harmony-optional-chaining --harmony-nullish tests/js/fflonk_setup_gpu.js
"use strict";
const fs = require("fs"), os = require("os"), path = require("path");
const ROOT = path.join(__dirname, "..", "..");
process.env.NTHREADS = process.env.NTHREADS || "8";
const snarkjs = require(path.join(ROOT, "oracle", "ref_shim.js"));
const { registerAll, unregister } = require(path.join(ROOT, "snarkjs_amd", "js", "register.js"));
const G = (f) => path.join(ROOT, "tests", "golden", f);
const bytes = (f) => new Uint8Array(fs.readFileSync(G(f)));
let fails = 0;
function check(name, ok, extra) { if (!ok) { fails++; console.log("FAIL", name, extra || ""); } else console.log("ok  ", name); }
const same = (a, b) => Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;
async function thrown(f) { try { await f(); } catch (e) { return e.message; } return null; }

async function main() {
    const orig = snarkjs.fflonk.setup;
    const golden = bytes("fflonk_setup_bn128_edge.zkey");
    // the reference on a BLS12-381 ceremony, before anything is registered: what opting in must not change
    const blsRef = { type: "mem" };
    await orig(bytes("plonk_setup_bls12381_tiny.r1cs"), bytes("setup_bls12381_p8.ptau"), blsRef);
    await registerAll(snarkjs);
    check("registerAll(snarkjs) keeps the reference's fflonk.setup", snarkjs.fflonk.setup === orig);
    await registerAll(snarkjs, { plonkSetup: true });
    check("{ plonkSetup: true } keeps the reference's fflonk.setup", snarkjs.fflonk.setup === orig);
    await registerAll(snarkjs, { fflonkSetup: true });
    check("{ fflonkSetup: true } replaces fflonk.setup", snarkjs.fflonk.setup !== orig);
    const tmp = path.join(fs.mkdtempSync(path.join(os.tmpdir(), "zkmi-fflonk-setup-")), "k.zkey");
    const logs = [];
    const logger = { error: (m) => logs.push("ERROR " + m), info: (m) => logs.push(m), debug() {} };
    let rc = await snarkjs.fflonk.setup(G("setup_bn128_edge.r1cs"), G("fflonk_setup_bn128_p12s.ptau"), tmp, logger);
    check("fflonk.setup to a path: the golden key", rc === 0 && same(new Uint8Array(fs.readFileSync(tmp)), golden));
    check("the reference's count lines", logs.includes("  Constraints:   176") && logs.includes("  Additions:     64"), logs.join("|"));
    const mem = { type: "mem" };
    rc = await snarkjs.fflonk.setup(bytes("setup_bn128_edge.r1cs"), { type: "mem", data: bytes("fflonk_setup_bn128_p12s.ptau") }, mem);
    check("fflonk.setup from bytes to a mem descriptor: the golden key", rc === 0 && same(mem.data, golden));
    let msg = await thrown(() => snarkjs.fflonk.setup(G("setup_bls12381_edge.r1cs"), G("setup_bn128_p8.ptau"), { type: "mem" }));
    check("curve mismatch: the reference's message", msg === "r1cs curve does not match powers of tau ceremony curve", msg);
    msg = await thrown(() => snarkjs.fflonk.setup(G("fflonk_setup_bn128_rows31.r1cs"), G("setup_bn128_p8.ptau"), { type: "mem" }));
    check("too small: the reference's message", msg === "Powers of Tau is not big enough for this circuit size. Section 2 too small.", msg);
    const bls = { type: "mem" };
    await snarkjs.fflonk.setup(bytes("plonk_setup_bls12381_tiny.r1cs"), bytes("setup_bls12381_p8.ptau"), bls);
    check("a BLS12-381 ceremony reaches the original function: the reference's bytes", same(bls.data, blsRef.data));
    unregister(snarkjs);
    check("unregister(snarkjs) restores the reference's fflonk.setup", snarkjs.fflonk.setup === orig);
    const ref = { type: "mem" };
    // the reference here is its browser bundle, which reads a string as a URL: hand it bytes
    await snarkjs.fflonk.setup(bytes("setup_bn128_edge.r1cs"), bytes("fflonk_setup_bn128_p12s.ptau"), ref);
    check("the reference path produces the golden key", same(ref.data, golden));
    fs.unlinkSync(tmp);
    console.log(fails ? `${fails} FAILED` : "ALL OK");
    process.exit(fails ? 1 : 0);
}
main().catch((e) => { console.error(e); process.exit(1); });
