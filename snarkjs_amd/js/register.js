// snarkjs_amd/js/register.js — makes unmodified snarkjs run its prover hot path on the MI355X.
//
// snarkjs reaches all bulk arithmetic through ONE object per curve, returned by getCurveFromName / getCurveFromQ /
// getCurveFromR (reference src/curves.js:9-53) and cached in globalThis.curve_bn128 / curve_bls12381 (bundle
// build/snarkjs.min.js:1@240638).  register(curve) replaces the bulk entry points of that object
//     curve.G1.multiExpAffine, curve.G2.multiExpAffine                       (min.js:1@214996)
//     curve.Fr.fft, curve.Fr.ifft                                             (min.js:1@215859)
//     curve.Fr.batchApplyKey / batchToMontgomery / batchFromMontgomery / batchInverse (min.js:1@211529, @188677)
// with calls into the HIP library through the N-API addon (../napi/zkmi_napi.node -> libzkmi.so, include/zkmi.h),
// keeping the reference's argument meaning, container rules (Uint8Array in -> Uint8Array out, BigBuffer in ->
// BigBuffer out, inputs never mutated) and error messages.  Everything else on the curve object (element-level
// Fr/G1/G2 ops, pairing, curve.tm, ceremony-only group FFTs) is left untouched.
//
// There is no silent fallback: without a HIP device register() throws.
"use strict";
const path = require("path");

const CURVE_ID = { bn128: 0, bls12381: 1 };
const OP = { TO_MONTGOMERY: 0, FROM_MONTGOMERY: 1, INVERSE: 2 };

function loadAddon() {
    return require(path.join(__dirname, "..", "napi", "zkmi_napi.node"));
}
function isBig(b) { return b && !(b instanceof Uint8Array) && Array.isArray(b.buffers) && typeof b.byteLength === "number"; }
function isBuf(b) { return (b instanceof Uint8Array) || isBig(b); }
// Uint8Array -> itself; BigBuffer -> its page list (ffjavascript BigBuffer.buffers)
function pagesOf(b) { return (b instanceof Uint8Array) ? b : b.buffers; }
// Result containers follow the reference function by function (downstream code tests `instanceof BigBuffer`, e.g.
// src/groth16_prove.js:361): batchToMontgomery / batchFromMontgomery / batchApplyKey return the input's own type
// (min.js:1 helper before @185893, @211529); fft / ifft / batchInverse first take `buff.slice(0, byteLength)`, which for a
// BigBuffer of at most one page is a plain Uint8Array (BigBuffer.slice, min.js:1@183423), and return THAT type.
const PAGE_SIZE = 1 << 30;
function allocLike(b, byteLength) { return new b.constructor(byteLength); }
function allocLikeSliced(b, byteLength) {
    return (b instanceof Uint8Array || b.byteLength <= PAGE_SIZE) ? new Uint8Array(byteLength) : new b.constructor(byteLength);
}
// Resident bases: the last argument of addon.msm only ALLOWS the library to keep a base buffer's pre-computed window tables on the
// device. Identity is established by the library itself from the full content of the buffer (include/zkmi.h: zkmi_msm) — never
// by a fingerprint computed here — and a table is only built the second time the same bytes are seen, under an LRU byte budget.
const CACHE_ALLOWED = 1;                                    // ZKMI_BASES_CACHE
// options.immutableBases: the caller's PROMISE that a base buffer it passes again (same memory, same length) still holds the same bytes — zkey
// sections and SRS slices that snarkjs reads once and never writes to. Only then the library re-checks a resident buffer by sample instead of
// hashing all of it on every call (include/zkmi.h: ZKMI_BASES_IMMUTABLE; saves ~0.6 ms of a 2^20-point call). Default false: the result of
// every call follows the bytes passed, as the reference's does, even if a buffer was edited in place between two calls.
const BASES_IMMUTABLE = 2;                                  // ZKMI_BASES_IMMUTABLE
function log2(n) { let l = 0; while ((1 << (l + 1)) <= n && l < 40) l++; return l; }

function register(curve, options) {
    options = options || {};
    const addon = options.addon || loadAddon();
    if (curve.__zkmi) return curve;
    const cid = CURVE_ID[curve.name];
    if (cid === undefined) throw new Error(`Curve not supported: ${curve.name}`);
    addon.init(options.device === undefined ? 0 : options.device);      // throws when no HIP device is visible
    const Fr = curve.Fr;
    const orig = {};
    const cacheBases = options.cacheBases !== false;      // keep base tables resident between calls (static zkey sections)
    const cacheMinPoints = options.cacheMinPoints === undefined ? 4096 : options.cacheMinPoints;
    const cacheBits = CACHE_ALLOWED | (options.immutableBases === true ? BASES_IMMUTABLE : 0);
    // options.async !== false: multiExpAffine / fft / ifft run on a libuv pool thread (addon.msmAsync / nttAsync, napi_create_async_work)
    // and the Node event loop keeps turning meanwhile; `async: false` keeps the blocking calls.
    const useAsync = options.async !== false && typeof addon.msmAsync === "function" && typeof addon.nttAsync === "function";
    // options.minPoints (default 0: every buffer-form call runs on the device): calls on FEWER elements go to the curve's own saved entry points
    // — the reference's WASM, the behaviour SURVEY.md 8b describes for a drop-in ("falls back to the saved originals when n is small"). A call on
    // 4 points costs the device path about a dozen launches (bench.py: wall_through_napi.msm_small_ms / ntt_small_ms); a host that issues
    // many tiny calls (a verifier's nPublic-point MSM in a loop) sets e.g. minPoints: 1024. Never applied silently: the default is 0.
    const minPoints = options.minPoints === undefined ? 0 : options.minPoints;

    for (const [gname, group] of [["G1", 1], ["G2", 2]]) {
        const G = curve[gname];
        orig[gname] = { multiExpAffine: G.multiExpAffine };
        G.multiExpAffine = async function (buffBases, buffScalars, logger, logText) {
            if (!isBuf(buffBases)) {
                if (logger) logger.error(`${logText} _multiExpChunk buffBases is not Uint8Array`);
                throw new Error(`${logText} _multiExpChunk buffBases is not Uint8Array`);
            }
            if (!isBuf(buffScalars)) {
                if (logger) logger.error(`${logText} _multiExpChunk buffScalars is not Uint8Array`);
                throw new Error(`${logText} _multiExpChunk buffScalars is not Uint8Array`);
            }
            const sGIn = G.F.n8 * 2;
            const nPoints = Math.floor(buffBases.byteLength / sGIn);
            if (nPoints == 0) return G.zero;
            const sScalar = Math.floor(buffScalars.byteLength / nPoints);
            if (sScalar * nPoints != buffScalars.byteLength) throw new Error("Scalar size does not match");
            if (nPoints < minPoints) return orig[gname].multiExpAffine.apply(G, arguments);
            if (logger) logger.debug(`Multiexp start: ${logText}: 0/${nPoints}`);
            const key = (cacheBases && nPoints >= cacheMinPoints) ? cacheBits : 0;
            const res = useAsync ? await addon.msmAsync(cid, group, pagesOf(buffBases), pagesOf(buffScalars), nPoints, sScalar, key)
                                 : addon.msm(cid, group, pagesOf(buffBases), pagesOf(buffScalars), nPoints, sScalar, key);
            if (logger) logger.debug(`Multiexp end: ${logText}: 0/${nPoints}`);
            return res;                                                  // Jacobian, Montgomery, 3*F.n8 bytes
        };
    }

    // Ceremony side (SURVEY.md 8 f4): G.fft / G.ifft over affine points (src/powersoftau_preparephase2.js:87 reaches G.ifft through
    // G.lagrangeEvaluations, which the reference implements on top of this very property for 2^k <= 2^Fr.s points) and
    // G.batchApplyKey (src/mpc_applykey.js:44-70). Only the affine -> affine forms the reference's callers use are taken over; any other
    // inType / outType combination, the array-of-elements form and sizes above 2^28 fall through to the WASM original.
    // The point-format conversions G.batchLEMtoU / batchUtoLEM / batchLEMtoC / batchCtoLEM of the ceremony files are taken over as well.
    // options.ceremony === false leaves all of these methods alone.
    if (options.ceremony !== false) {
        for (const [gname, group] of [["G1", 1], ["G2", 2]]) {
            const G = curve[gname], sG = G.F.n8 * 2;
            Object.assign(orig[gname], { fft: G.fft, ifft: G.ifft, batchApplyKey: G.batchApplyKey });
            const gfft = (inverse, origFn) => async function (buff, inType, outType, logger, loggerTxt) {
                inType = inType || "affine"; outType = outType || "affine";
                if (!isBuf(buff) || inType !== "affine" || outType !== "affine") return origFn.apply(G, arguments);
                const n = buff.byteLength / sG, bits = log2(n);
                if ((1 << bits) != n) throw new Error("fft must be multiple of 2");
                if (bits > 28 || bits > Fr.s) return origFn.apply(G, arguments);
                const out = allocLikeSliced(buff, buff.byteLength);
                addon.groupFft(cid, group, pagesOf(buff), pagesOf(out), bits, inverse ? 1 : 0);
                return out;
            };
            if (typeof G.fft === "function") { G.fft = gfft(false, orig[gname].fft); G.ifft = gfft(true, orig[gname].ifft); }
            // Point-format conversions of the ceremony files (helper `Ia`, min.js:1 before @185893: output has the input's own container
            // type, "Invalid buffer size" when the length is not a whole number of points): LEM <-> U, LEM <-> C.
            for (const [name, kind, sIn, sOut] of [["batchLEMtoU", 0, sG, sG], ["batchUtoLEM", 1, sG, sG], ["batchLEMtoC", 2, sG, sG / 2], ["batchCtoLEM", 3, sG / 2, sG]]) {
                if (typeof G[name] !== "function") continue;
                orig[gname][name] = G[name];
                G[name] = async function (buff) {
                    if (!isBuf(buff)) return orig[gname][name].apply(G, arguments);
                    const n = Math.floor(buff.byteLength / sIn);
                    if (n * sIn !== buff.byteLength) throw new Error("Invalid buffer size");
                    const out = allocLike(buff, n * sOut);
                    addon.groupConvert(cid, group, kind, pagesOf(buff), pagesOf(out), n);
                    return out;
                };
            }
            if (typeof G.batchApplyKey === "function") {
                G.batchApplyKey = async function (buff, first, inc, inType, outType) {
                    inType = inType || "affine"; outType = outType || "affine";
                    if (!isBuf(buff) || inType !== "affine" || outType !== "affine") return orig[gname].batchApplyKey.apply(G, arguments);
                    const n = Math.floor(buff.byteLength / sG);
                    const out = allocLike(buff, n * sG);
                    addon.groupApplyKey(cid, group, pagesOf(buff), pagesOf(out), n, Fr.e(first), Fr.e(inc));
                    return out;
                };
            }
        }
    }

    orig.Fr = { fft: Fr.fft, ifft: Fr.ifft, batchApplyKey: Fr.batchApplyKey, batchToMontgomery: Fr.batchToMontgomery,
                batchFromMontgomery: Fr.batchFromMontgomery, batchInverse: Fr.batchInverse };

    async function ntt(buff, inverse, origFn, args) {
        if (Array.isArray(buff)) return origFn.apply(Fr, args);          // array-of-elements form: not on the prove path
        if (!isBuf(buff)) throw new Error("fft: buffer is not Uint8Array or BigBuffer");
        const n = buff.byteLength / Fr.n8;
        const bits = log2(n);
        if ((1 << bits) != n) throw new Error("fft must be multiple of 2");
        // n = 2^(Fr.s+1): the reference's "extended" transform over the quadratic extension's root (min.js:1@216148) is not built on the device;
        // like the group FFTs above, such a call goes to the saved WASM entry point instead of failing
        if (n < minPoints || bits > Fr.s) return origFn.apply(Fr, args);
        const out = allocLikeSliced(buff, buff.byteLength);
        if (useAsync) await addon.nttAsync(cid, pagesOf(buff), pagesOf(out), bits, inverse ? 1 : 0, null, null);
        else addon.ntt(cid, pagesOf(buff), pagesOf(out), bits, inverse ? 1 : 0, null, null);
        return out;
    }
    Fr.fft = function (buff, inType, outType, logger, loggerTxt) { return ntt(buff, false, orig.Fr.fft, arguments); };
    Fr.ifft = function (buff, inType, outType, logger, loggerTxt) { return ntt(buff, true, orig.Fr.ifft, arguments); };

    Fr.batchApplyKey = async function (buff, first, inc, inType, outType) {
        if (!isBuf(buff) || buff.byteLength / Fr.n8 < minPoints) return orig.Fr.batchApplyKey.apply(Fr, arguments);
        const out = allocLike(buff, buff.byteLength);
        addon.applyKey(cid, pagesOf(buff), pagesOf(out), Math.floor(buff.byteLength / Fr.n8), Fr.e(first), Fr.e(inc));
        return out;
    };
    function batch(op, name) {
        return async function (buff) {
            if (!isBuf(buff)) return orig.Fr[name].apply(Fr, arguments);
            if (buff.byteLength % Fr.n8) throw new Error("Invalid buffer size");
            if (buff.byteLength / Fr.n8 < minPoints) return orig.Fr[name].apply(Fr, arguments);
            const out = (op == OP.INVERSE ? allocLikeSliced : allocLike)(buff, buff.byteLength);
            addon.frBatch(cid, op, pagesOf(buff), pagesOf(out), Math.floor(buff.byteLength / Fr.n8));
            return out;
        };
    }
    Fr.batchToMontgomery = batch(OP.TO_MONTGOMERY, "batchToMontgomery");
    Fr.batchFromMontgomery = batch(OP.FROM_MONTGOMERY, "batchFromMontgomery");
    Fr.batchInverse = batch(OP.INVERSE, "batchInverse");

    curve.__zkmi = { addon, cid, orig };
    return curve;
}

// Undo register(): restore the reference WASM entry points (used by A/B parity tests).
function unregister(curve) {
    if (curve && curve.__zkmiWtnsCheck) uninstallWtnsCheck(curve);              // unregister(snarkjs): wtns.check of registerAll(snarkjs, { wtnsCheck: true })
    if (curve && curve.__zkmiPtauChallenge) uninstallPtauChallenge(curve);      // unregister(snarkjs): exportChallenge / challengeContribute / importResponse of registerAll(snarkjs, { ptauChallenge: true })
    if (curve && curve.__zkmiPtauContribute) uninstallPtauContribute(curve);    // unregister(snarkjs): newAccumulator / contribute / beacon of registerAll(snarkjs, { ptauContribute: true })
    if (curve && curve.__zkmiPtauPrepare) uninstallPtauPrepare(curve);          // unregister(snarkjs): preparePhase2 / convert of registerAll(snarkjs, { ptauPrepare: true })
    if (curve && curve.__zkmiPtauVerify) uninstallPtauVerify(curve);            // unregister(snarkjs): powersOfTau.verify of registerAll(snarkjs, { ptauVerify: true })
    if (curve && curve.__zkmiBellman) uninstallBellman(curve);                  // unregister(snarkjs): exportBellman / bellmanContribute / importBellman of registerAll(snarkjs, { bellman: true })
    if (curve && curve.__zkmiPhase2Verify) uninstallPhase2Verify(curve);    // unregister(snarkjs): verifyFromInit / verifyFromR1cs of registerAll(snarkjs, { phase2Verify: true })
    if (curve && curve.__zkmiPhase2) uninstallPhase2(curve);            // unregister(snarkjs): contribute / beacon of registerAll(snarkjs, { phase2: true }), before the setup gives the namespace back
    if (curve && curve.__zkmiSetup) uninstallSetup(curve);              // unregister(snarkjs): the setup replacement installed by registerAll(snarkjs, { setup: true })
    if (curve && curve.__zkmiPlonkSetup) uninstallPlonkSetup(curve);    // and the one installed by registerAll(snarkjs, { plonkSetup: true })
    if (curve && curve.__zkmiFflonkSetup) uninstallFflonkSetup(curve);  // and by registerAll(snarkjs, { fflonkSetup: true })
    if (!curve.__zkmi) return curve;
    const o = curve.__zkmi.orig;
    Object.assign(curve.G1, o.G1);
    Object.assign(curve.G2, o.G2);
    Object.assign(curve.Fr, o.Fr);
    delete curve.__zkmi;
    return curve;
}

// Patch both curves through snarkjs's own getter so that the cached instances are the ones patched.
// options.fused (r06): ALSO put the fused provers behind snarkjs's own prover entry points (installFused below).
async function registerAll(snarkjs, options) {
    const out = {};
    for (const name of ["bn128", "bls12381"]) out[name] = register(await snarkjs.curves.getCurveFromName(name), options);
    if (options && options.fused) out.fused = installFused(snarkjs, options);
    if (options && options.setup) out.setup = installSetup(snarkjs, options);
    if (options && options.plonkSetup) out.plonkSetup = installPlonkSetup(snarkjs, options);
    if (options && options.fflonkSetup) out.fflonkSetup = installFflonkSetup(snarkjs, options);
    if (options && options.phase2) out.phase2 = installPhase2(snarkjs, options);
    if (options && options.phase2Verify) out.phase2Verify = installPhase2Verify(snarkjs, options);
    if (options && options.bellman) out.bellman = installBellman(snarkjs, options);
    if (options && options.ptauVerify) out.ptauVerify = installPtauVerify(snarkjs, options);
    if (options && options.ptauPrepare) out.ptauPrepare = installPtauPrepare(snarkjs, options);
    if (options && options.ptauContribute) out.ptauContribute = installPtauContribute(snarkjs, options);
    if (options && options.ptauChallenge) out.ptauChallenge = installPtauChallenge(snarkjs, options);
    if (options && options.wtnsCheck) out.wtnsCheck = installWtnsCheck(snarkjs, options);
    return out;
}

// ---- wtns.check on the device (opt-in: registerAll(snarkjs, { wtnsCheck: true })) ---------------------------------------------------------------------------
// The reference's check is one JavaScript loop over the constraints that no curve method sees, so like the fused provers it is replaced through the writable
// PROPERTY snarkjs.wtns (js/wtns_check_native.js). Same arguments (paths, fastfile descriptors, in-memory files), verdict and info / warn lines; a bad witness
// with no logger throws the reference's TypeError. Handed to the saved reference function, before a line is logged or the device is touched: every input the
// reference refuses or reads beyond a buffer for (js/wtns_check_native.js lists them). options.dev replaces the device calls.
function installWtnsCheck(snarkjs, options) {
    if (snarkjs.__zkmiWtnsCheck) return snarkjs.__zkmiWtnsCheck;
    const wtnsN = require("./wtns_check_native.js");
    const saved = { check: snarkjs.wtns.check };
    let dev = options && options.dev;
    if (!dev) {
        const addon = (options && options.addon) || loadAddon();
        addon.init(options && options.device !== undefined ? options.device : 0);
        dev = wtnsN.deviceOf(addon);
    }
    async function check(r1csFilename, wtnsFilename, logger) {
        try {
            return await wtnsN.check(r1csFilename, wtnsFilename, logger, { dev });
        } catch (e) {
            if (e instanceof wtnsN.WtnsRefusal && e.handOver) return saved.check(r1csFilename, wtnsFilename, logger);
            throw e;
        }
    }
    snarkjs.wtns = Object.freeze(Object.assign({}, snarkjs.wtns, { check }));
    snarkjs.__zkmiWtnsCheck = { saved };
    return snarkjs.__zkmiWtnsCheck;
}
function uninstallWtnsCheck(snarkjs) {
    if (!snarkjs.__zkmiWtnsCheck) return;
    snarkjs.wtns = Object.freeze(Object.assign({}, snarkjs.wtns, snarkjs.__zkmiWtnsCheck.saved));
    delete snarkjs.__zkmiWtnsCheck;
}

// ---- zKey.newZKey on the device (opt-in: registerAll(snarkjs, { setup: true })) ---------------------------------------------------------------------
// newZKey sends its task lists straight to the workers (src/zkey_new.js:338-577), so patching the curve object cannot reach it; like the fused provers it
// is replaced through the writable PROPERTY snarkjs.zKey. Same signature, inputs (paths, bytes, fastfile descriptors) and result: csHash, or -1 with the
// reference's logger.error where the reference refuses. One call is handed to the saved reference function: a domain of 2^15 or more that equals the
// ceremony's power (js/groth16_setup_native.js: the reference's circuit hash reads past the tauG1 section there; INTEGRATION.md 1c).
function installSetup(snarkjs, options) {
    if (snarkjs.__zkmiSetup) return snarkjs.__zkmiSetup;
    const setupN = require("./groth16_setup_native.js");
    const orig = snarkjs.zKey;
    const addon = (options && options.addon) || loadAddon();
    addon.init(options && options.device !== undefined ? options.device : 0);
    async function newZKey(r1csName, ptauName, zkeyName, logger) {
        let res;
        try { res = setupN.newZKey(r1csName, ptauName, { addon }); } catch (e) {
            if (e instanceof setupN.SetupRefusal) {
                if (e.handOver) return orig.newZKey(r1csName, ptauName, zkeyName, logger);
                if (e.throws) throw new Error(e.message);
                if (logger) logger.error(e.message);
                return -1;
            }
            throw e;
        }
        if (typeof zkeyName === "string") require("fs").writeFileSync(zkeyName, res.zkey);
        else if (zkeyName && zkeyName.type === "file") require("fs").writeFileSync(zkeyName.fileName, res.zkey);
        else if (zkeyName && zkeyName.type === "mem") zkeyName.data = res.zkey;
        else throw new Error("newZKey: expected a path or a fastfile descriptor for the new key");
        if (logger) logger.info("Circuit hash: " + Buffer.from(res.csHash).toString("hex"));
        return res.csHash;
    }
    snarkjs.zKey = Object.freeze(Object.assign({}, orig, { newZKey }));
    snarkjs.__zkmiSetup = { orig };
    return snarkjs.__zkmiSetup;
}
function uninstallSetup(snarkjs) {
    if (!snarkjs.__zkmiSetup) return;
    snarkjs.zKey = snarkjs.__zkmiSetup.orig;
    delete snarkjs.__zkmiSetup;
}

// ---- zKey.contribute / zKey.beacon on the device (opt-in: registerAll(snarkjs, { phase2: true })) ------------------------------------------------------
// Through the patched curve methods a contribution feeds G.batchApplyKey 2^16 points at a time (src/mpc_applykey.js:29-51), an upload, a launch of the
// general kernel and a download per chunk; here sections L and H are one call each of the one-scalar kernel (js/groth16_phase2_native.js). Replaced
// through the writable PROPERTY snarkjs.zKey like newZKey: same arguments, the same draw of 64 bytes (globalThis.crypto.getRandomValues where the
// reference's browser build uses it), same result: the contribution hash; beacon returns false with the reference's logger.error where it refuses.
// Handed to the saved reference function: an empty entropy (the reference asks for one), a point section larger than one buffer, and a name whose
// UTF-8 form overflows the one-byte length field.
function installPhase2(snarkjs, options) {
    if (snarkjs.__zkmiPhase2) return snarkjs.__zkmiPhase2;
    const phase2N = require("./groth16_phase2_native.js");
    const saved = { contribute: snarkjs.zKey.contribute, beacon: snarkjs.zKey.beacon };
    const addon = (options && options.addon) || loadAddon();
    addon.init(options && options.device !== undefined ? options.device : 0);
    const hex = (b) => Buffer.from(b).toString("hex");
    function store(zkeyName, zkey, what) {
        if (typeof zkeyName === "string") require("fs").writeFileSync(zkeyName, zkey);
        else if (zkeyName && zkeyName.type === "file") require("fs").writeFileSync(zkeyName.fileName, zkey);
        else if (zkeyName && zkeyName.type === "mem") zkeyName.data = zkey;
        else throw new Error(what + ": expected a path or a fastfile descriptor for the new key");
    }
    async function contribute(zkeyNameOld, zkeyNameNew, name, entropy, logger) {
        if (!entropy) return saved.contribute(zkeyNameOld, zkeyNameNew, name, entropy, logger);
        let res;
        try {
            const random64 = new Uint8Array(64);
            if (globalThis.crypto && globalThis.crypto.getRandomValues) globalThis.crypto.getRandomValues(random64); else require("crypto").randomFillSync(random64);
            res = phase2N.contribute(zkeyNameOld, name, entropy, { addon, random64 });
        } catch (e) {
            if (e instanceof phase2N.Phase2Refusal && e.handOver) return saved.contribute(zkeyNameOld, zkeyNameNew, name, entropy, logger);
            if (e instanceof phase2N.Phase2Refusal) throw new Error(e.message);
            throw e;
        }
        store(zkeyNameNew, res.zkey, "zKey.contribute");
        if (logger) { logger.info("Circuit Hash: " + hex(res.csHash)); logger.info("Contribution Hash: " + hex(res.contributionHash)); }
        return res.contributionHash;
    }
    async function beacon(zkeyNameOld, zkeyNameNew, name, beaconHashStr, numIterationsExp, logger) {
        let res;
        try { res = phase2N.beacon(zkeyNameOld, name, beaconHashStr, numIterationsExp, { addon }); } catch (e) {
            if (e instanceof phase2N.Phase2Refusal && e.handOver) return saved.beacon(zkeyNameOld, zkeyNameNew, name, beaconHashStr, numIterationsExp, logger);
            if (e instanceof phase2N.Phase2Refusal && e.throws) throw new Error(e.message);
            if (e instanceof phase2N.Phase2Refusal) { if (logger) logger.error(e.message); return false; }
            throw e;
        }
        store(zkeyNameNew, res.zkey, "zKey.beacon");
        if (logger) logger.info("Contribution Hash: " + hex(res.contributionHash));
        return res.contributionHash;
    }
    // the namespace object in place now may already be the setup's copy (installSetup): keep whatever it holds, replace these two alone
    snarkjs.zKey = Object.freeze(Object.assign({}, snarkjs.zKey, { contribute, beacon }));
    snarkjs.__zkmiPhase2 = { saved };
    return snarkjs.__zkmiPhase2;
}
function uninstallPhase2(snarkjs) {
    if (!snarkjs.__zkmiPhase2) return;
    snarkjs.zKey = Object.freeze(Object.assign({}, snarkjs.zKey, snarkjs.__zkmiPhase2.saved));
    delete snarkjs.__zkmiPhase2;
}

// ---- zKey.exportBellman / bellmanContribute / importBellman on the device (opt-in: registerAll(snarkjs, { bellman: true })) ---------------------------------
// Through the patched curve methods the H basis change of these calls does not reach the device (G.fft / G.ifft / G.batchApplyKey with a jacobian form are
// forwarded to WASM); here it is one call each way (js/groth16_bellman_native.js). Same arguments, the same draw of 64 bytes, the same bytes in the new file,
// the same result (undefined, the contribution hash, true) and logger lines; importBellman returns false with the reference's logger.error where it refuses.
// Handed to the saved reference function: whatever the driver marks handOver (a file that is not well-formed or too short, a section beyond one buffer, an
// unknown curve, an empty entropy, ...). Combines with setup, phase2 and phase2Verify: each replaces its own members of the copy of snarkjs.zKey.
function installBellman(snarkjs, options) {
    if (snarkjs.__zkmiBellman) return snarkjs.__zkmiBellman;
    const bN = require("./groth16_bellman_native.js");
    const saved = { exportBellman: snarkjs.zKey.exportBellman, bellmanContribute: snarkjs.zKey.bellmanContribute, importBellman: snarkjs.zKey.importBellman };
    const addon = (options && options.addon) || loadAddon();
    addon.init(options && options.device !== undefined ? options.device : 0);
    const dev = options && options.dev;
    const logOf = (logger) => (level, text) => { if (logger && typeof logger[level] === "function") logger[level](text); };
    function store(target, raw, what) {
        if (typeof target === "string") require("fs").writeFileSync(target, raw);
        else if (target && target.type === "file") require("fs").writeFileSync(target.fileName, raw);
        else if (target && target.type === "mem") target.data = raw;
        else throw new Error(what + ": expected a path or a fastfile descriptor for the new file");
    }
    // run the driver; null: the call goes to the saved function; false: the reference's logged refusal
    async function attempt(f, logger) {
        try { return await f(); } catch (e) {
            if (!(e instanceof bN.BellmanRefusal)) throw e;
            if (e.handOver) return null;
            if (e.returnsFalse) { if (logger) logger.error(e.message); return false; }
            throw new Error(e.message);
        }
    }
    async function exportBellman(zkeyName, mpcparamsName, logger) {
        const res = await attempt(() => bN.exportBellman(zkeyName, { addon, dev }), logger);
        if (res === null) return saved.exportBellman(zkeyName, mpcparamsName, logger);
        store(mpcparamsName, res.params, "zKey.exportBellman");
    }
    async function bellmanContribute(curve, challengeFilename, responseFileName, entropy, logger) {
        if (!entropy) return saved.bellmanContribute(curve, challengeFilename, responseFileName, entropy, logger);
        const random64 = new Uint8Array(64);
        if (globalThis.crypto && globalThis.crypto.getRandomValues) globalThis.crypto.getRandomValues(random64); else require("crypto").randomFillSync(random64);
        const res = await attempt(() => bN.bellmanContribute(curve, challengeFilename, entropy, { addon, dev, random64, log: logOf(logger) }), logger);
        // the saved function draws its own 64 bytes: a pinned stream differs from the reference's by this one draw, on calls the driver does not take
        if (res === null) return saved.bellmanContribute(curve, challengeFilename, responseFileName, entropy, logger);
        store(responseFileName, res.response, "zKey.bellmanContribute");
        return res.contributionHash;
    }
    async function importBellman(zkeyNameOld, mpcparamsName, zkeyNameNew, name, logger) {
        const res = await attempt(() => bN.importBellman(zkeyNameOld, mpcparamsName, name, { addon, dev }), logger);
        if (res === null) return saved.importBellman(zkeyNameOld, mpcparamsName, zkeyNameNew, name, logger);
        if (res === false) return false;
        store(zkeyNameNew, res.zkey, "zKey.importBellman");
        return true;
    }
    snarkjs.zKey = Object.freeze(Object.assign({}, snarkjs.zKey, { exportBellman, bellmanContribute, importBellman }));
    snarkjs.__zkmiBellman = { saved };
    return snarkjs.__zkmiBellman;
}
function uninstallBellman(snarkjs) {
    if (!snarkjs.__zkmiBellman) return;
    snarkjs.zKey = Object.freeze(Object.assign({}, snarkjs.zKey, snarkjs.__zkmiBellman.saved));
    delete snarkjs.__zkmiBellman;
}

// ---- zKey.verifyFromInit / zKey.verifyFromR1cs on the device (opt-in: registerAll(snarkjs, { phase2Verify: true })) -----------------------------------
// Through the patched curve methods the verification reaches the device in chunks of 2^20 points, an upload and a download each, and two of its loops not at
// all: the H check draws domainSize - 1 field elements one at a time from a generator in JavaScript, and batchSubtract sends g1m_subAffine task lists straight
// to the workers. Here the same-ratio checks of a key are one launch, and the two sums of the L and of the H check one call each
// (js/groth16_phase2_verify_native.js). Same arguments, the same verdict, the same lines to console.log and the logger. Handed to the saved reference
// function: a section beyond one 2^30-byte buffer, power >= Fr.s, inputs the readers do not take, and for verifyFromR1cs what the device newZKey leaves to it.
function installPhase2Verify(snarkjs, options) {
    if (snarkjs.__zkmiPhase2Verify) return snarkjs.__zkmiPhase2Verify;
    const verifyN = require("./groth16_phase2_verify_native.js");
    const saved = { verifyFromInit: snarkjs.zKey.verifyFromInit, verifyFromR1cs: snarkjs.zKey.verifyFromR1cs };
    const addon = (options && options.addon) || loadAddon();
    addon.init(options && options.device !== undefined ? options.device : 0);
    const run = (which) => async function (firstName, pTauFileName, zkeyFileName, logger) {
        const log = (level, text) => { if (level === "log") console.log(text); else if (logger) logger[level](text); };
        try {
            const random64 = new Uint8Array(64);
            if (globalThis.crypto && globalThis.crypto.getRandomValues) globalThis.crypto.getRandomValues(random64); else require("crypto").randomFillSync(random64);
            return await verifyN[which](firstName, pTauFileName, zkeyFileName, { addon, log, random64 });
        } catch (e) {
            if (e instanceof verifyN.Phase2Refusal && e.handOver) return saved[which](firstName, pTauFileName, zkeyFileName, logger);
            if (e instanceof verifyN.Phase2Refusal) throw new Error(e.message);
            throw e;
        }
    };
    snarkjs.zKey = Object.freeze(Object.assign({}, snarkjs.zKey, { verifyFromInit: run("verifyFromInit"), verifyFromR1cs: run("verifyFromR1cs") }));
    snarkjs.__zkmiPhase2Verify = { saved };
    return snarkjs.__zkmiPhase2Verify;
}
function uninstallPhase2Verify(snarkjs) {
    if (!snarkjs.__zkmiPhase2Verify) return;
    snarkjs.zKey = Object.freeze(Object.assign({}, snarkjs.zKey, snarkjs.__zkmiPhase2Verify.saved));
    delete snarkjs.__zkmiPhase2Verify;
}

// ---- powersOfTau.verify on the device (opt-in: registerAll(snarkjs, { ptauVerify: true })) -----------------------------------------------------------------
// Through the patched curve methods the check reaches the device in chunks of 2^16 points, an upload and a download each, with JavaScript loops over the
// generator for every power of every section and one WASM pairing per sameRatio. Here a section is one call and all same-ratio checks one launch
// (js/powersoftau_verify_native.js). Same argument, verdict and info / warn / error lines. Handed to the saved reference function: a section beyond one
// 2^30-byte buffer, power + 1 > Fr.s, inputs the readers do not take.
function installPtauVerify(snarkjs, options) {
    if (snarkjs.__zkmiPtauVerify) return snarkjs.__zkmiPtauVerify;
    const verifyN = require("./powersoftau_verify_native.js");
    const saved = { verify: snarkjs.powersOfTau.verify };
    const addon = (options && options.addon) || loadAddon();
    addon.init(options && options.device !== undefined ? options.device : 0);
    async function verify(tauFilename, logger) {
        const log = (level, text) => { if (logger) logger[level](text); };
        try {
            const random32 = new Uint8Array(32);
            if (globalThis.crypto && globalThis.crypto.getRandomValues) globalThis.crypto.getRandomValues(random32); else require("crypto").randomFillSync(random32);
            return await verifyN.verify(tauFilename, { addon, log, random32 });
        } catch (e) {
            if (e instanceof verifyN.PtauRefusal && e.handOver) return saved.verify(tauFilename, logger);
            if (e instanceof verifyN.PtauRefusal) throw new Error(e.message);
            throw e;
        }
    }
    snarkjs.powersOfTau = Object.freeze(Object.assign({}, snarkjs.powersOfTau, { verify }));
    snarkjs.__zkmiPtauVerify = { saved };
    return snarkjs.__zkmiPtauVerify;
}
function uninstallPtauVerify(snarkjs) {
    if (!snarkjs.__zkmiPtauVerify) return;
    snarkjs.powersOfTau = Object.freeze(Object.assign({}, snarkjs.powersOfTau, snarkjs.__zkmiPtauVerify.saved));
    delete snarkjs.__zkmiPtauVerify;
}

// ---- powersOfTau.preparePhase2 / convert on the device (opt-in: registerAll(snarkjs, { ptauPrepare: true })) ----------------------------------------------
// Through the patched curve methods preparePhase2 reaches the device once per power and section: G.lagrangeEvaluations -> G.ifft with an upload, p + 2 launches
// and a download each, and a re-read of the source section in between. Here a section is one call that transforms all its powers in one pass
// (js/powersoftau_prepare_native.js). Same arguments and the same bytes in the new file; both return undefined like the reference. Handed to the saved reference
// function: any file that is not well-formed, power + 1 > Fr.s, a section beyond one 2^30-byte buffer, inputs the readers do not take.
function installPtauPrepare(snarkjs, options) {
    if (snarkjs.__zkmiPtauPrepare) return snarkjs.__zkmiPtauPrepare;
    const prepareN = require("./powersoftau_prepare_native.js");
    const saved = { preparePhase2: snarkjs.powersOfTau.preparePhase2, convert: snarkjs.powersOfTau.convert };
    const addon = (options && options.addon) || loadAddon();
    addon.init(options && options.device !== undefined ? options.device : 0);
    const run = (which) => async function (oldPtauFilename, newPTauFilename, logger) {
        let raw;
        try { raw = await prepareN[which](oldPtauFilename, { addon }); } catch (e) {
            if (e instanceof prepareN.PrepareRefusal && e.handOver) return saved[which](oldPtauFilename, newPTauFilename, logger);
            throw e;
        }
        if (typeof newPTauFilename === "string") require("fs").writeFileSync(newPTauFilename, raw);
        else if (newPTauFilename && newPTauFilename.type === "file") require("fs").writeFileSync(newPTauFilename.fileName, raw);
        else if (newPTauFilename && newPTauFilename.type === "mem") newPTauFilename.data = raw;
        else throw new Error("powersOfTau." + which + ": expected a path or a fastfile descriptor for the new file");
    };
    // the namespace object in place now may already be the verifier's copy (installPtauVerify): keep whatever it holds, replace these two alone
    snarkjs.powersOfTau = Object.freeze(Object.assign({}, snarkjs.powersOfTau, { preparePhase2: run("preparePhase2"), convert: run("convert") }));
    snarkjs.__zkmiPtauPrepare = { saved };
    return snarkjs.__zkmiPtauPrepare;
}
function uninstallPtauPrepare(snarkjs) {
    if (!snarkjs.__zkmiPtauPrepare) return;
    snarkjs.powersOfTau = Object.freeze(Object.assign({}, snarkjs.powersOfTau, snarkjs.__zkmiPtauPrepare.saved));
    delete snarkjs.__zkmiPtauPrepare;
}

// ---- powersOfTau.newAccumulator / contribute / beacon on the device (opt-in: registerAll(snarkjs, { ptauContribute: true })) --------------------------------
// Through the patched curve methods a contribution feeds G.batchApplyKey and the two conversions 2^20 / sG points at a time, an upload, a launch of the general
// kernel and a download each; here a section is one call (js/powersoftau_contribute_native.js). Same arguments, the same draw of 64 bytes
// (globalThis.crypto.getRandomValues where the reference's browser build uses it), the same bytes in the new file, the same result: the response hash
// (newAccumulator: the first challenge hash); beacon returns false with the reference's logger.error where it refuses. Handed to the saved reference function:
// whatever the driver marks handOver (a file that is not well-formed, power 0, an empty entropy, a section beyond one buffer, ...).
function installPtauContribute(snarkjs, options) {
    if (snarkjs.__zkmiPtauContribute) return snarkjs.__zkmiPtauContribute;
    const contribN = require("./powersoftau_contribute_native.js");
    const saved = { newAccumulator: snarkjs.powersOfTau.newAccumulator, contribute: snarkjs.powersOfTau.contribute, beacon: snarkjs.powersOfTau.beacon };
    const addon = (options && options.addon) || loadAddon();
    addon.init(options && options.device !== undefined ? options.device : 0);
    const dev = options && options.dev;
    const logOf = (logger) => (level, text) => { if (logger && typeof logger[level] === "function") logger[level](text); };
    function store(target, raw, what) {
        if (typeof target === "string") require("fs").writeFileSync(target, raw);
        else if (target && target.type === "file") require("fs").writeFileSync(target.fileName, raw);
        else if (target && target.type === "mem") target.data = raw;
        else throw new Error(what + ": expected a path or a fastfile descriptor for the new file");
    }
    // run the driver; null: the call goes to the saved function
    async function attempt(f, logger) {
        try { return await f(); } catch (e) {
            if (!(e instanceof contribN.ContributeRefusal)) throw e;
            if (e.handOver) return null;
            if (e.throws) throw new Error(e.message);
            if (!e.logged && logger) logger.error(e.message);
            return false;
        }
    }
    async function newAccumulator(curve, power, fileName, logger) {
        const res = await attempt(() => contribN.newAccumulator(curve, power, { log: logOf(logger) }), logger);
        if (res === null) return saved.newAccumulator(curve, power, fileName, logger);
        store(fileName, res.ptau, "powersOfTau.newAccumulator");
        return res.firstChallengeHash;
    }
    async function contribute(oldPtauFilename, newPTauFilename, name, entropy, logger) {
        if (!entropy) return saved.contribute(oldPtauFilename, newPTauFilename, name, entropy, logger);
        const random64 = new Uint8Array(64);
        if (globalThis.crypto && globalThis.crypto.getRandomValues) globalThis.crypto.getRandomValues(random64); else require("crypto").randomFillSync(random64);
        const res = await attempt(() => contribN.contribute(oldPtauFilename, name, entropy, { addon, dev, random64, log: logOf(logger) }), logger);
        // the saved function draws its own 64 bytes: a pinned stream differs from the reference's by this one draw, on calls the reference fails or refuses anyway
        if (res === null) return saved.contribute(oldPtauFilename, newPTauFilename, name, entropy, logger);
        store(newPTauFilename, res.ptau, "powersOfTau.contribute");
        return res.responseHash;
    }
    async function beacon(oldPtauFilename, newPTauFilename, name, beaconHashStr, numIterationsExp, logger) {
        const res = await attempt(() => contribN.beacon(oldPtauFilename, name, beaconHashStr, numIterationsExp, { addon, dev, log: logOf(logger) }), logger);
        if (res === null) return saved.beacon(oldPtauFilename, newPTauFilename, name, beaconHashStr, numIterationsExp, logger);
        if (res === false) return false;
        store(newPTauFilename, res.ptau, "powersOfTau.beacon");
        return res.responseHash;
    }
    // the namespace object in place now may already be another installer's copy: keep whatever it holds, replace these three alone
    snarkjs.powersOfTau = Object.freeze(Object.assign({}, snarkjs.powersOfTau, { newAccumulator, contribute, beacon }));
    snarkjs.__zkmiPtauContribute = { saved };
    return snarkjs.__zkmiPtauContribute;
}
function uninstallPtauContribute(snarkjs) {
    if (!snarkjs.__zkmiPtauContribute) return;
    snarkjs.powersOfTau = Object.freeze(Object.assign({}, snarkjs.powersOfTau, snarkjs.__zkmiPtauContribute.saved));
    delete snarkjs.__zkmiPtauContribute;
}

// ---- powersOfTau.exportChallenge / challengeContribute / importResponse on the device (opt-in: registerAll(snarkjs, { ptauChallenge: true })) -----------------
// A section is one call (js/powersoftau_challenge_native.js). Same arguments, the same draw of 64 bytes, the same bytes in the new file, the same result
// (the challenge hash, undefined, the next challenge hash) and the reference's errors. Handed to the saved reference function: whatever the driver marks
// handOver (a file that is not well-formed, power 0 in importResponse, an empty entropy, a section beyond one buffer, ...).
function installPtauChallenge(snarkjs, options) {
    if (snarkjs.__zkmiPtauChallenge) return snarkjs.__zkmiPtauChallenge;
    const chN = require("./powersoftau_challenge_native.js");
    const saved = { exportChallenge: snarkjs.powersOfTau.exportChallenge, challengeContribute: snarkjs.powersOfTau.challengeContribute, importResponse: snarkjs.powersOfTau.importResponse };
    const addon = (options && options.addon) || loadAddon();
    addon.init(options && options.device !== undefined ? options.device : 0);
    const dev = options && options.dev;
    const logOf = (logger) => (level, text) => { if (logger && typeof logger[level] === "function") logger[level](text); };
    const nameOf = (src) => (typeof src === "string" ? src : (src && src.fileName));
    function store(target, raw, what) {
        if (typeof target === "string") require("fs").writeFileSync(target, raw);
        else if (target && target.type === "file") require("fs").writeFileSync(target.fileName, raw);
        else if (target && target.type === "mem") target.data = raw;
        else throw new Error(what + ": expected a path or a fastfile descriptor for the new file");
    }
    // run the driver; null: the call goes to the saved function
    async function attempt(f, onThrow) {
        try { return await f(); } catch (e) {
            if (!(e instanceof chN.ChallengeRefusal)) throw e;
            if (e.handOver) return null;
            if (onThrow) onThrow(e);
            throw new Error(e.message);
        }
    }
    async function exportChallenge(pTauFilename, challengeFilename, logger) {
        const res = await attempt(() => chN.exportChallenge(pTauFilename, { addon, dev, log: logOf(logger), fileName: nameOf(pTauFilename) }),
                                  (e) => { if (e.challenge) store(challengeFilename, e.challenge, "powersOfTau.exportChallenge"); });
        if (res === null) return saved.exportChallenge(pTauFilename, challengeFilename, logger);
        store(challengeFilename, res.challenge, "powersOfTau.exportChallenge");
        return res.challengeHash;
    }
    async function challengeContribute(curve, challengeFilename, responseFileName, entropy, logger) {
        if (!entropy) return saved.challengeContribute(curve, challengeFilename, responseFileName, entropy, logger);
        const random64 = new Uint8Array(64);
        if (globalThis.crypto && globalThis.crypto.getRandomValues) globalThis.crypto.getRandomValues(random64); else require("crypto").randomFillSync(random64);
        const res = await attempt(() => chN.challengeContribute(curve, challengeFilename, entropy, { addon, dev, random64, log: logOf(logger) }));
        // the saved function draws its own 64 bytes: a pinned stream differs from the reference's by this one draw, on calls the driver does not take
        if (res === null) return saved.challengeContribute(curve, challengeFilename, responseFileName, entropy, logger);
        store(responseFileName, res.response, "powersOfTau.challengeContribute");
    }
    async function importResponse(oldPtauFilename, contributionFilename, newPTauFilename, name, importPoints, logger) {
        const res = await attempt(() => chN.importResponse(oldPtauFilename, contributionFilename, name, importPoints, { addon, dev, log: logOf(logger) }));
        if (res === null) return saved.importResponse(oldPtauFilename, contributionFilename, newPTauFilename, name, importPoints, logger);
        store(newPTauFilename, res.ptau, "powersOfTau.importResponse");
        return res.nextChallenge;
    }
    snarkjs.powersOfTau = Object.freeze(Object.assign({}, snarkjs.powersOfTau, { exportChallenge, challengeContribute, importResponse }));
    snarkjs.__zkmiPtauChallenge = { saved };
    return snarkjs.__zkmiPtauChallenge;
}
function uninstallPtauChallenge(snarkjs) {
    if (!snarkjs.__zkmiPtauChallenge) return;
    snarkjs.powersOfTau = Object.freeze(Object.assign({}, snarkjs.powersOfTau, snarkjs.__zkmiPtauChallenge.saved));
    delete snarkjs.__zkmiPtauChallenge;
}

// ---- plonk.setup on the device (opt-in: registerAll(snarkjs, { plonkSetup: true }); { setup: true } stays Groth16 only) ------------------------------
// plonk.setup reaches the device through the patched curve methods alone for its transforms and multiexps; the gate lowering, the permutation, the Lagrange
// section and the selector buffers stay single-threaded JavaScript (src/plonk_setup.js). Replaced through the writable PROPERTY snarkjs.plonk: same
// signature, inputs and result (undefined, or -1 with the reference's logger.error where the reference refuses).
function installPlonkSetup(snarkjs, options) {
    if (snarkjs.__zkmiPlonkSetup) return snarkjs.__zkmiPlonkSetup;
    const setupN = require("./plonk_setup_native.js");
    const addon = (options && options.addon) || loadAddon();
    addon.init(options && options.device !== undefined ? options.device : 0);
    const saved = snarkjs.plonk.setup;
    async function setup(r1csName, ptauName, zkeyName, logger) {
        let zkey;
        try { zkey = setupN.setup(r1csName, ptauName, { addon, logger }); } catch (e) {
            if (e instanceof setupN.SetupRefusal) { if (logger) logger.error(e.message); return -1; }
            throw e;
        }
        if (typeof zkeyName === "string") require("fs").writeFileSync(zkeyName, zkey);
        else if (zkeyName && zkeyName.type === "file") require("fs").writeFileSync(zkeyName.fileName, zkey);
        else if (zkeyName && zkeyName.type === "mem") zkeyName.data = zkey;
        else throw new Error("plonk.setup: expected a path or a fastfile descriptor for the new key");
        if (logger) logger.info("Setup Finished");
    }
    // the namespace object in place now may already be the fused provers' copy (installFused): keep whatever it holds, replace setup alone
    snarkjs.plonk = Object.freeze(Object.assign({}, snarkjs.plonk, { setup }));
    snarkjs.__zkmiPlonkSetup = { saved };
    return snarkjs.__zkmiPlonkSetup;
}
function uninstallPlonkSetup(snarkjs) {
    if (!snarkjs.__zkmiPlonkSetup) return;
    snarkjs.plonk = Object.freeze(Object.assign({}, snarkjs.plonk, { setup: snarkjs.__zkmiPlonkSetup.saved }));
    delete snarkjs.__zkmiPlonkSetup;
}

// ---- fflonk.setup on the device (opt-in: registerAll(snarkjs, { fflonkSetup: true })), BN254 -----------------------------------------------------------
// Like plonk.setup, fflonk.setup reaches the device through the patched curve methods for its transforms and its one multiexp only; the gate lowering,
// writeQMap, writeSigma, the Lagrange section and the CPolynomial interleave stay single-threaded JavaScript (src/fflonk_setup.js). Replaced through the
// writable PROPERTY snarkjs.fflonk: same signature, inputs and result (0; where the reference refuses it throws, and so does this, with the same words).
// A ceremony on any curve but bn128 goes to the original function: the reference writes BN254's roots into such a key, and opting in changes nothing there.
function installFflonkSetup(snarkjs, options) {
    if (snarkjs.__zkmiFflonkSetup) return snarkjs.__zkmiFflonkSetup;
    const setupN = require("./fflonk_setup_native.js");
    const addon = (options && options.addon) || loadAddon();
    addon.init(options && options.device !== undefined ? options.device : 0);
    const saved = snarkjs.fflonk.setup;
    async function setup(r1csName, ptauName, zkeyName, logger) {
        if (!setupN.isBn128(ptauName)) return saved(r1csName, ptauName, zkeyName, logger);
        let zkey;
        try { zkey = setupN.setup(r1csName, ptauName, { addon, logger }); } catch (e) {
            if (e instanceof setupN.SetupRefusal) throw new Error(e.message);
            throw e;
        }
        if (typeof zkeyName === "string") require("fs").writeFileSync(zkeyName, zkey);
        else if (zkeyName && zkeyName.type === "file") require("fs").writeFileSync(zkeyName.fileName, zkey);
        else if (zkeyName && zkeyName.type === "mem") zkeyName.data = zkey;
        else throw new Error("fflonk.setup: expected a path or a fastfile descriptor for the new key");
        if (logger) logger.info("FFLONK SETUP FINISHED");
        return 0;
    }
    snarkjs.fflonk = Object.freeze(Object.assign({}, snarkjs.fflonk, { setup }));
    snarkjs.__zkmiFflonkSetup = { saved };
    return snarkjs.__zkmiFflonkSetup;
}
function uninstallFflonkSetup(snarkjs) {
    if (!snarkjs.__zkmiFflonkSetup) return;
    snarkjs.fflonk = Object.freeze(Object.assign({}, snarkjs.fflonk, { setup: snarkjs.__zkmiFflonkSetup.saved }));
    delete snarkjs.__zkmiFflonkSetup;
}

// ---- the fused provers behind snarkjs.groth16 / plonk / fflonk (opt-in: registerAll(snarkjs, { fused: true })) ------------------------------------
// Patching the curve object leaves the reference's own JavaScript around the bulk calls: at 2^20 constraints snarkjs.groth16.prove then takes 2.6 s, 0.08 s of
// it on the device (buildABC1, src/groth16_prove.js:147-187, is a single-threaded loop of per-element WASM calls). The prover functions themselves are reached
// through the module object — `snarkjs.groth16` is a frozen namespace, but the PROPERTY snarkjs.groth16 is writable — so a caller of
// snarkjs.groth16.prove / fullProve, snarkjs.plonk.prove / fullProve, snarkjs.fflonk.prove / fullProve gets the fused device provers (js/groth16_native.js,
// plonk_native.js, fflonk_native.js) with the reference's signature, inputs (paths, bytes, fastfile descriptors), blinding draws (curve.Fr.random, in the
// reference's order) and outputs: same proof for the same draws (tests/js/unmodified_gpu.js step 6). Keys stay resident per zkey (path or buffer identity).
// What is NOT redirected: snarkjs's own CLI (its action table calls the prover functions directly, not through the namespace) and
// `{ singleThread: true }` calls, which keep their private WASM curve. uninstallFused(snarkjs) restores the namespaces and frees the keys.
function installFused(snarkjs, options) {
    if (snarkjs.__zkmiFused) return snarkjs.__zkmiFused;
    const fs = require("fs");
    const { makeProver } = require("./groth16_native.js");
    const plonkN = require("./plonk_native.js"), fflonkN = require("./fflonk_native.js");
    const orig = { groth16: snarkjs.groth16, plonk: snarkjs.plonk, fflonk: snarkjs.fflonk };
    const prover = makeProver(snarkjs, options);
    const keys = new Map();                                  // PLONK / FFLONK keys resident per zkey source
    const idOf = (src) => (typeof src === "string" ? "file:" + src : (src && src.type === "file" ? "file:" + src.fileName : (src && src.type === "mem" ? src.data : src)));
    const bytesOf = (src) => {
        if (typeof src === "string") return new Uint8Array(fs.readFileSync(src));
        if (src instanceof Uint8Array) return src;
        if (src && src.type === "file") return new Uint8Array(fs.readFileSync(src.fileName));
        if (src && src.type === "mem") return (src.data instanceof Uint8Array) ? src.data : src.data.slice(0, src.data.byteLength);
        throw new Error("expected a path, the file's bytes or a fastfile descriptor");
    };
    const residentKey = (Cls, src) => {
        const id = idOf(src);
        let k = keys.get(id);
        if (!k) { k = new Cls(bytesOf(src), options); keys.set(id, k); }
        return k;
    };
    const single = (o) => !!(o && o.singleThread);
    async function polyProve(mod, Cls, nDraws, zkey, wtns) {
        const key = residentKey(Cls, zkey);
        const curve = await snarkjs.curves.getCurveFromName(key.curveName);
        const draws = [];
        for (let i = 0; i < nDraws; i++) draws.push(Uint8Array.from(curve.Fr.random()));     // src/plonk_prove.js:222-227 / src/fflonk_prove.js:321-324: all draws first, in order
        return mod.proveAsync(key, bytesOf(wtns), draws);
    }
    const fullOf = (prove) => async function (input, wasmFile, zkey, logger, wtnsCalcOptions, proverOptions) {      // src/groth16_fullprove.js:24-33 and its twins
        const wtns = { type: "mem" };
        await snarkjs.wtns.calculate(input, wasmFile, wtns, wtnsCalcOptions);
        return prove(zkey, wtns, logger, proverOptions);
    };
    const g16 = (zkey, wtns, logger, o) => (single(o) ? orig.groth16.prove(zkey, wtns, logger, o) : prover.prove(zkey, wtns));
    const pl = (zkey, wtns, logger, o) => (single(o) ? orig.plonk.prove(zkey, wtns, logger, o) : polyProve(plonkN, plonkN.PlonkKey, 11, zkey, wtns));
    const ff = (zkey, wtns, logger, o) => (single(o) ? orig.fflonk.prove(zkey, wtns, logger, o) : polyProve(fflonkN, fflonkN.FflonkKey, 9, zkey, wtns));
    // options.verify: snarkjs.groth16.verify on the device as well (js/groth16_verify_native.js: batches of concurrent calls, keys per vk content)
    // options.verify as an object picks the protocols: { groth16: true, plonk: true } (verifyPlonk: true is the same as verify.plonk); `verify: true` alone keeps
    // meaning Groth16 only, and snarkjs.plonk.verify then stays the reference's (js/plonk_verify_native.js otherwise). { fflonk: true } (alias verifyFflonk: true) does
    // the same for snarkjs.fflonk.verify (js/fflonk_verify_native.js, BN254 only)
    const vopt = options && options.verify, vobj = vopt && typeof vopt === "object";
    const verifier = (vobj ? vopt.groth16 : vopt) ? require("./groth16_verify_native.js").makeVerifier(snarkjs, options) : null;
    const plonkVerifier = (vobj && vopt.plonk) || (options && options.verifyPlonk) ? require("./plonk_verify_native.js").makeVerifier(snarkjs, options) : null;
    const fflonkVerifier = (vobj && vopt.fflonk) || (options && options.verifyFflonk) ? require("./fflonk_verify_native.js").makeVerifier(snarkjs, options) : null;
    snarkjs.groth16 = Object.freeze(Object.assign({}, orig.groth16, { prove: g16, fullProve: fullOf(g16) }, verifier ? { verify: verifier.verify } : {}));
    snarkjs.plonk = Object.freeze(Object.assign({}, orig.plonk, { prove: pl, fullProve: fullOf(pl) }, plonkVerifier ? { verify: plonkVerifier.verify } : {}));
    snarkjs.fflonk = Object.freeze(Object.assign({}, orig.fflonk, { prove: ff, fullProve: fullOf(ff) }, fflonkVerifier ? { verify: fflonkVerifier.verify } : {}));
    snarkjs.__zkmiFused = { orig, prover, keys, verifier, plonkVerifier, fflonkVerifier };
    return snarkjs.__zkmiFused;
}
async function uninstallFused(snarkjs) {
    const st = snarkjs.__zkmiFused;
    if (!st) return;
    snarkjs.groth16 = st.orig.groth16; snarkjs.plonk = st.orig.plonk; snarkjs.fflonk = st.orig.fflonk;
    delete snarkjs.__zkmiFused;
    for (const k of st.keys.values()) { try { k.release(); } catch (e) { /* already released */ } }
    st.keys.clear();
    if (st.verifier) st.verifier.release();
    if (st.plonkVerifier) st.plonkVerifier.release();
    if (st.fflonkVerifier) st.fflonkVerifier.release();
    await st.prover.release();
}

module.exports = { register, unregister, registerAll, installFused, uninstallFused, installSetup, uninstallSetup, installPlonkSetup, uninstallPlonkSetup, installFflonkSetup, uninstallFflonkSetup, installPhase2, uninstallPhase2, installPhase2Verify, uninstallPhase2Verify, installBellman, uninstallBellman, installPtauVerify, uninstallPtauVerify, installPtauPrepare, uninstallPtauPrepare, installPtauContribute, uninstallPtauContribute, installPtauChallenge, uninstallPtauChallenge, installWtnsCheck, uninstallWtnsCheck, loadAddon };
