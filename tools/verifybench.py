"""Batch Groth16 verification rate on one GPU: verifications/s through VerifyingKey.verify_many (from the JSON objects) and through
verify_raw (packed arrays, no parsing) for BN254 and BLS12-381 at several batch sizes, the verification kernel's device time per proof (HIP
events: zkmi_groth16_verify_last_ms), and, in the same run and outside the timed windows, the reference's own single-thread WASM verify rate
on this host (tools/ref_wasm_verify.js through the bundle in oracle/_ref/). --protocol plonk does the same for PLONK (snarkjs_amd.plonk_verify, sizes 1 /
64 / 4 096, batches of DISTINCT device proofs: see main_plonk) next to the reference's WASM plonk.verify, and measures the Groth16 verify rate at batch 4 096 in the same run: the PLONK rate is expected
not to fall below half of it (`plonk_vs_groth16_4096`). Warm-up first, then `reps` timed windows per point; the JSON line
reports the median and the spread. --protocol fflonk (BN254; snarkjs_amd.fflonk_verify, main_fflonk) reports the FFLONK rate on batches of distinct device
proofs next to three yardsticks of the same run: the reference's WASM fflonk.verify, and this library's PLONK and Groth16 verify rates at batch 4 096. The batches hold the golden proof in distinct encodings (Jacobian z = 2 + i for entry i), so every lane
decodes different bytes; the publics, and so the vk_x double-and-add, are the same in every lane. Prints one JSON line."""
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]


def rate(fn, n, reps):
    fn()                                                    # warm-up
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return {"per_s": round(n / statistics.median(ts), 1), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5)}


def wasm_baseline(count, protocol="groth16"):
    node = shutil.which("node")
    script = os.path.join(ROOT, "tools", "ref_wasm_verify.js")
    if node is None or not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "build", "snarkjs.min.js")):
        return None
    r = subprocess.run([node, "--harmony-optional-chaining", "--harmony-nullish", script, str(count)] + ([protocol] if protocol != "groth16" else []), capture_output=True, text=True, timeout=900)
    return json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else {"error": r.stderr[-500:]}


def main():
    import verify_vectors as V
    import groth16_verify_oracle as O
    import numpy as np
    from snarkjs_amd import groth16_verify, zkmi
    sizes = [int(x) for x in os.environ.get("VERIFYBENCH_SIZES", "1,64,4096,65536").split(",")]
    reps = int(os.environ.get("VERIFYBENCH_REPS", "3"))
    out = {"what": "groth16 batch verify", "reps": reps, "wasm_single_thread": wasm_baseline(int(os.environ.get("VERIFYBENCH_WASM_COUNT", "40"))), "curves": {}}
    for f in ("groth16_bn128_n1024.json", "groth16_bls12381_n1024.json"):
        vk, pubs, proof = V.golden(f)
        E = O.BN254 if vk["curve"] == "bn128" else O.BLS12381
        key = groth16_verify.VerifyingKey(vk)
        base = [V.jacobian(E, proof, 2 + i, 3 + i) for i in range(min(max(sizes), 4096))]
        res = {}
        for n in sizes:
            proofs = (base * (n // len(base) + 1))[:n]
            lists = [pubs] * n
            recs, pu, ns, _ = key.pack(lists, proofs) if n <= 4096 else (None, None, None, None)
            if recs is None:
                r4, p4, ns, _ = key.pack([pubs] * len(base), base)
                reps_n = n // len(base)
                recs, pu = np.tile(r4, reps_n), np.tile(p4, reps_n)
            entry = {"verify_many": rate(lambda: key.verify_many(lists, proofs), n, reps) if n <= 4096 else None,
                     "verify_raw": rate(lambda: key.verify_raw(recs, pu, ns, n), n, reps)}
            kms = zkmi.lib().zkmi_groth16_verify_last_ms()
            entry["kernel_ms"] = round(kms, 3)
            entry["kernel_us_per_proof"] = round(1000.0 * kms / n, 3)
            assert all(c == 1 for c in key.verify_raw(recs, pu, ns, n))
            res[str(n)] = entry
        wasm = (out["wasm_single_thread"] or {}).get(vk["curve"])
        if wasm and "4096" in res:
            res["ratio_verify_many_4096_vs_wasm"] = round(res["4096"]["verify_many"]["per_s"] / wasm["per_s"], 1)
        out["curves"][vk["curve"]] = res
        key.release()
    print(json.dumps(out))


def main_plonk():
    """Headline batches hold DISTINCT valid proofs: `VERIFYBENCH_DISTINCT` (256) device proofs of the golden witness, each with fresh blinding, so
    that the lanes of a wavefront carry different challenges and different Straus scalars (entry i is proof i mod 256: any 64 consecutive lanes
    differ) and the additions of B1 cost what they cost in use. `uniform_4096` is the same measurement on one proof in distinct encodings, where all
    lanes of a wavefront agree on every scalar bit: the divergence-free best case, kept beside it."""
    import plonk_verify_vectors as PV
    import verify_vectors as V
    import groth16_verify_oracle as O
    from snarkjs_amd import groth16_verify, plonk, plonk_verify, zkmi
    sizes = [int(x) for x in os.environ.get("VERIFYBENCH_SIZES", "1,64,4096").split(",")]
    reps = int(os.environ.get("VERIFYBENCH_REPS", "3"))
    n_distinct = max(64, int(os.environ.get("VERIFYBENCH_DISTINCT", "256")))
    out = {"what": "plonk batch verify", "reps": reps, "distinct_proofs": n_distinct,
           "wasm_single_thread": wasm_baseline(int(os.environ.get("VERIFYBENCH_WASM_COUNT", "40")), "plonk"), "curves": {}}
    gd = os.path.join(ROOT, "tests", "golden")
    for tag, g16 in (("plonk_bn128_n2048", "groth16_bn128_n1024.json"), ("plonk_bls12381_small", "groth16_bls12381_n1024.json")):
        vk, pubs, proof = PV.golden(tag + ".json")
        E = PV.curve_of(vk)
        pkey = plonk.PlonkKey(open(os.path.join(gd, tag + ".zkey"), "rb").read())
        wtns = open(os.path.join(gd, tag + ".wtns"), "rb").read()
        distinct = [plonk.prove(pkey, wtns)["proof"] for _ in range(n_distinct)]
        pkey.release()
        assert len({p["Wxi"][0] for p in distinct}) == n_distinct
        key = plonk_verify.VerifyingKey(vk)

        def point(proofs, n):
            lists = [pubs] * n
            recs, pu, ns, _ = key.pack(lists, proofs)
            entry = {"verify_many": rate(lambda: key.verify_many(lists, proofs), n, reps), "verify_raw": rate(lambda: key.verify_raw(recs, pu, ns, n), n, reps)}
            kms = zkmi.lib().zkmi_plonk_verify_last_ms()
            entry["kernel_ms"] = round(kms, 3)
            entry["kernel_us_per_proof"] = round(1000.0 * kms / n, 3)
            assert all(c == 1 for c in key.verify_raw(recs, pu, ns, n))
            return entry
        res = {str(n): point([distinct[i % n_distinct] for i in range(n)], n) for n in sizes}
        # one proof 4 096 times, one commitment per entry in a distinct Jacobian encoding (z = 2 + i): every lane of a wavefront takes the same branches
        res["uniform_4096"] = point([PV.with_(proof, **{PV.POINTS[i % 9]: PV.jacobian(E, PV.affine(E, proof[PV.POINTS[i % 9]]), 2 + i)}) for i in range(4096)], 4096)
        key.release()
        # the same device's Groth16 verify rate at batch 4 096, same run
        gvk, gpubs, gproof = V.golden(g16)
        GE = O.BN254 if gvk["curve"] == "bn128" else O.BLS12381
        gkey = groth16_verify.VerifyingKey(gvk)
        gproofs = [V.jacobian(GE, gproof, 2 + i, 3 + i) for i in range(4096)]
        grecs, gpu, gns, _ = gkey.pack([gpubs] * 4096, gproofs)
        res["groth16_4096"] = {"verify_many": rate(lambda: gkey.verify_many([gpubs] * 4096, gproofs), 4096, reps), "verify_raw": rate(lambda: gkey.verify_raw(grecs, gpu, gns, 4096), 4096, reps)}
        gkey.release()
        if "4096" in res:
            res["plonk_vs_groth16_4096"] = {k: round(res["4096"][k]["per_s"] / res["groth16_4096"][k]["per_s"], 3) for k in ("verify_many", "verify_raw")}
        wasm = (out["wasm_single_thread"] or {}).get(vk["curve"])
        if wasm and "4096" in res:
            res["ratio_verify_many_4096_vs_wasm"] = round(res["4096"]["verify_many"]["per_s"] / wasm["per_s"], 1)
        out["curves"][vk["curve"]] = res
    print(json.dumps(out))


def main_fflonk():
    """As main_plonk, for FFLONK on BN254: `VERIFYBENCH_DISTINCT` (256) device proofs of the golden witness with fresh blinding each, tiled to the batch size;
    `uniform_4096` is one proof repeated (one commitment per entry in a distinct Jacobian encoding): no divergence in the Straus sum; size 1 is the
    latency of one proof alone. In the same run: PLONK on 256 distinct device proofs tiled to 4 096 and Groth16 at 4 096 (the golden proof in distinct
    encodings), and `fflonk_vs_plonk_4096` / `fflonk_vs_groth16_4096`."""
    import fflonk_verify_vectors as FV
    import plonk_verify_vectors as PV
    import verify_vectors as V
    import groth16_verify_oracle as O
    from snarkjs_amd import fflonk, fflonk_verify, groth16_verify, plonk, plonk_verify, zkmi
    sizes = [int(x) for x in os.environ.get("VERIFYBENCH_SIZES", "1,64,4096").split(",")]
    reps = int(os.environ.get("VERIFYBENCH_REPS", "5"))
    n_distinct = max(64, int(os.environ.get("VERIFYBENCH_DISTINCT", "256")))
    out = {"what": "fflonk batch verify", "reps": reps, "distinct_proofs": n_distinct,
           "wasm_single_thread": wasm_baseline(int(os.environ.get("VERIFYBENCH_WASM_COUNT", "40")), "fflonk"), "curves": {}}
    gd = os.path.join(ROOT, "tests", "golden")
    L = zkmi.lib()

    def point(key, last_ms, lists, proofs):
        n = len(proofs)
        recs, pu, ns, _ = key.pack(lists, proofs)
        entry = {"verify_many": rate(lambda: key.verify_many(lists, proofs), n, reps), "verify_raw": rate(lambda: key.verify_raw(recs, pu, ns, n), n, reps)}
        kms = last_ms()
        entry["kernel_ms"] = round(kms, 3)
        entry["kernel_us_per_proof"] = round(1000.0 * kms / n, 3)
        assert all(c == 1 for c in key.verify_raw(recs, pu, ns, n))
        return entry
    tag = "fflonk_bn128_n256"
    vk, pubs, proof = FV.golden(tag + ".json")
    res_all = fflonk.prove_many(open(os.path.join(gd, tag + ".zkey"), "rb").read(), [open(os.path.join(gd, tag + ".wtns"), "rb").read()] * n_distinct)
    distinct = [r["proof"] for r in res_all]
    assert len({p["polynomials"]["W2"][0] for p in distinct}) == n_distinct
    key = fflonk_verify.VerifyingKey(vk)
    res = {str(n): point(key, L.zkmi_fflonk_verify_last_ms, [pubs] * n, [distinct[i % n_distinct] for i in range(n)]) for n in sizes}
    res["uniform_4096"] = point(key, L.zkmi_fflonk_verify_last_ms, [pubs] * 4096,
                                [FV.with_point(proof, FV.POINTS[i % 4], FV.jacobian(FV.affine(proof["polynomials"][FV.POINTS[i % 4]]), 2 + i)) for i in range(4096)])
    key.release()
    # yardstick: PLONK on distinct device proofs, batch 4 096, same run
    ptag = "plonk_bn128_n2048"
    pvk, ppubs, _ = PV.golden(ptag + ".json")
    pkey = plonk.PlonkKey(open(os.path.join(gd, ptag + ".zkey"), "rb").read())
    pw = open(os.path.join(gd, ptag + ".wtns"), "rb").read()
    pdistinct = [plonk.prove(pkey, pw)["proof"] for _ in range(n_distinct)]
    pkey.release()
    vkey = plonk_verify.VerifyingKey(pvk)
    res["plonk_4096"] = point(vkey, L.zkmi_plonk_verify_last_ms, [ppubs] * 4096, [pdistinct[i % n_distinct] for i in range(4096)])
    vkey.release()
    # yardstick: Groth16, batch 4 096, same run
    gvk, gpubs, gproof = V.golden("groth16_bn128_n1024.json")
    gkey = groth16_verify.VerifyingKey(gvk)
    res["groth16_4096"] = point(gkey, L.zkmi_groth16_verify_last_ms, [gpubs] * 4096, [V.jacobian(O.BN254, gproof, 2 + i, 3 + i) for i in range(4096)])
    gkey.release()
    if "4096" in res:
        for other in ("plonk", "groth16"):
            res[f"fflonk_vs_{other}_4096"] = {k: round(res["4096"][k]["per_s"] / res[other + "_4096"][k]["per_s"], 3) for k in ("verify_many", "verify_raw")}
        wasm = (out["wasm_single_thread"] or {}).get("bn128")
        if wasm:
            res["ratio_verify_many_4096_vs_wasm"] = round(res["4096"]["verify_many"]["per_s"] / wasm["per_s"], 1)
    out["curves"]["bn128"] = res
    print(json.dumps(out))


def main_aggregate(protocol):
    """--aggregate: the aggregated check (verify_all_raw) beside the per-proof path (verify_raw) of the same key, in one run on one device, on the same
    `VERIFYBENCH_DISTINCT` (256) distinct device proofs tiled to the batch (VERIFYBENCH_SIZES, default 4096,65536,262144): packed calls per
    second both ways, the per-proof kernel's HIP-event time, and the aggregated path's split into lane phase, reduction and tail."""
    import numpy as np
    import fflonk_verify_vectors as FV
    import plonk_verify_vectors as PV
    import verify_vectors as V
    from snarkjs_amd import fflonk, fflonk_verify, groth16, groth16_verify, plonk, plonk_verify, zkmi
    sizes = [int(x) for x in os.environ.get("VERIFYBENCH_SIZES", "4096,65536,262144").split(",")]
    reps = int(os.environ.get("VERIFYBENCH_REPS", "3"))
    n_distinct = max(64, int(os.environ.get("VERIFYBENCH_DISTINCT", "256")))
    out = {"what": protocol + " aggregated batch verify vs per-proof verify_raw", "reps": reps, "distinct_proofs": n_distinct, "curves": {}}
    gd = os.path.join(ROOT, "tests", "golden")
    L = zkmi.lib()
    tags = {"groth16": ("groth16_bn128_n1024", "groth16_bls12381_n1024"), "plonk": ("plonk_bn128_n2048", "plonk_bls12381_small"), "fflonk": ("fflonk_bn128_n256",)}[protocol]
    vec, prover, mod = {"groth16": (V, groth16, groth16_verify), "plonk": (PV, plonk, plonk_verify), "fflonk": (FV, fflonk, fflonk_verify)}[protocol]
    for tag in tags:
        vk, pubs, _ = vec.golden(tag + ".json")
        zkey, wtns = open(os.path.join(gd, tag + ".zkey"), "rb").read(), open(os.path.join(gd, tag + ".wtns"), "rb").read()
        if protocol == "groth16":                           # fresh (r, s) per proof: every pi_b differs
            pk = groth16.ProvingKey(zkey)
            distinct = [groth16.prove(pk, wtns)["proof"] for _ in range(n_distinct)]
            pk.release()
            assert len({tuple(p["pi_b"][0]) for p in distinct}) == n_distinct
        else:
            distinct = [r["proof"] for r in prover.prove_many(zkey, [wtns] * n_distinct)]
        key = mod.VerifyingKey(vk)
        r1, p1, ns, _ = key.pack([pubs] * n_distinct, distinct)
        res = {}
        for n in sizes:
            tiles = (n + n_distinct - 1) // n_distinct
            recs, pu = np.tile(r1, tiles)[:n * key.record_bytes], np.tile(p1, tiles)[:n * ns * 32]
            seed = bytes(range(32))
            entry = {"verify_raw": rate(lambda: key.verify_raw(recs, pu, ns, n), n, reps)}
            entry["per_proof_kernel_ms"] = round(getattr(L, "zkmi_%s_verify_last_ms" % protocol)(), 3)
            entry["verify_all_raw"] = rate(lambda: key.verify_all_raw(recs, pu, ns, n, seed), n, reps)
            ms = (zkmi.C.c_double * 3)()
            zkmi.check(getattr(L, "zkmi_%s_aggregate_phase_ms" % protocol)(ms))
            entry["aggregate_ms"] = {"lane": round(ms[0], 3), "reduce": round(ms[1], 3), "tail": round(ms[2], 3)}
            entry["lane_vs_per_proof_kernel"] = round(ms[0] / entry["per_proof_kernel_ms"], 3)
            entry["aggregate_vs_per_proof_rate"] = round(entry["verify_all_raw"]["per_s"] / entry["verify_raw"]["per_s"], 3)
            ok, codes = key.verify_all_raw(recs, pu, ns, n, seed)
            assert ok and (codes == 1).all()
            res[str(n)] = entry
        key.release()
        out["curves"][vk.get("curve", "bn128")] = res
    print(json.dumps(out))


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--protocol", choices=["groth16", "plonk", "fflonk"], default="groth16")
    ap.add_argument("--aggregate", action="store_true", help="the aggregated check beside the per-proof path of the same key")
    args = ap.parse_args()
    if args.aggregate:
        main_aggregate(args.protocol)
    else:
        {"groth16": main, "plonk": main_plonk, "fflonk": main_fflonk}[args.protocol]()
