"""Batch Groth16 verification rate on one GPU: verifications/s through VerifyingKey.verify_many (from the JSON objects) and through
verify_raw (packed arrays, no parsing) for BN254 and BLS12-381 at several batch sizes, the verification kernel's device time per proof (HIP
events: zkmi_groth16_verify_last_ms), and, in the same run and outside the timed windows, the reference's own single-thread WASM verify rate
on this host (tools/ref_wasm_verify.js through the bundle in oracle/_ref/). Warm-up first, then `reps` timed windows per point; the JSON line
reports the median and the spread. The batches hold the golden proof in distinct encodings (Jacobian z = 2 + i for entry i), so every lane
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


def wasm_baseline(count):
    node = shutil.which("node")
    script = os.path.join(ROOT, "tools", "ref_wasm_verify.js")
    if node is None or not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "build", "snarkjs.min.js")):
        return None
    r = subprocess.run([node, "--harmony-optional-chaining", "--harmony-nullish", script, str(count)], capture_output=True, text=True, timeout=900)
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


if __name__ == "__main__":
    main()
