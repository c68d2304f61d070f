"""Groth16 phase-2 verification (zkey verify): the generator on the device against the host's sequential draws, and the whole verification against the reference.

    python tools/phase2verifybench.py [--lg 20] [--reps 12] [--whole-min-lg 12] [--whole-max-lg 14] [--curve bn128] [--threads 16] [--out result.json]

(a) Generator alone, both curves, n = 2^lg results of Fr.fromRng: zkmi_chacha_fr_dev (wall time of the call, which ends with the stream idle; 2 warm-ups, the median of
--reps) against the host's sequential field_from_rng loop (zkmi_chacha_fr_host, one core, the median of 3) in the same process. The two outputs must be the same bytes.
(b) Whole call, --curve, domains 2^whole-min-lg .. 2^whole-max-lg: a key from tools/setupbench.py's generator (circuit-shaped r1cs, trapdoor ptau, device newZKey) plus one
device contribute, then the reference's WASM zKey.verifyFromInit (tools/phase2verifybench_ref.js, --threads worker threads) against groth16_phase2_verify.verify_from_init on
the same three files, on the same box, in the same run: a warm-up and the median of 5 each; both verdicts must be true. Needs node and the reference bundle staged in
oracle/_ref; without them (b) is reported as not measured."""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from snarkjs_amd import groth16_phase2 as p2, groth16_phase2_verify as pv, groth16_setup as gs, zkmi  # noqa: E402


def generator_leg(curve, lg, reps):
    cv = next(c for c in gs.CURVES.values() if c["name"] == curve)
    cid, n, L = cv["id"], 1 << lg, zkmi.lib()
    seed = (C.c_uint32 * 8)(*range(0x51, 0x59))
    d = zkmi.DeviceBuffer(32 * n)
    w_dev, w_host = C.c_uint64(), C.c_uint64()

    def device():
        t0 = time.perf_counter()
        zkmi.check(L.zkmi_chacha_fr_dev(cid, seed, d.ptr, n, C.byref(w_dev)))
        return (time.perf_counter() - t0) * 1e3
    for _ in range(2):
        device()
    td = [device() for _ in range(reps)]
    host = np.zeros(32 * n, np.uint8)
    th = []
    for _ in range(3):
        t0 = time.perf_counter()
        zkmi.check(L.zkmi_chacha_fr_host(cid, seed, zkmi.ptr(host), n, C.byref(w_host)))
        th.append((time.perf_counter() - t0) * 1e3)
    same = d.to_host().tobytes() == host.tobytes() and w_dev.value == w_host.value
    d.free()
    row = dict(leg="generator", curve=curve, lg=lg, reps=reps, device_ms=round(statistics.median(td), 3), device_min_max=[round(min(td), 3), round(max(td), 3)],
               host_sequential_ms=round(statistics.median(th), 3), host_min_max=[round(min(th), 3), round(max(th), 3)], words_consumed=w_dev.value, same_bytes=same)
    row["ratio"] = round(row["host_sequential_ms"] / row["device_ms"], 1)
    if not same:
        raise SystemExit(f"the device stream differs from the host's: {json.dumps(row)}")
    return row


def whole_leg(curve, lg, tmp, node, threads):
    import setupbench
    from snarkjs_amd.workloads import synth_r1cs
    r1_path, pt_path, init_path, key_path = (os.path.join(tmp, f"c{lg}.{e}") for e in ("r1cs", "ptau", "init.zkey", "zkey"))
    data, n_vars = synth_r1cs.circuit_shaped(curve, lg)
    open(r1_path, "wb").write(data)
    setupbench.trapdoor_ptau(curve, lg, pt_path)
    init, _cs = gs.new_zkey(r1_path, pt_path)
    key, _h = p2.contribute(init, "bench", "Entropy", bytes(range(64)))
    open(init_path, "wb").write(init)
    open(key_path, "wb").write(key)
    p = subprocess.run([node, "--harmony-optional-chaining", "--harmony-nullish", "--max-old-space-size=16384", os.path.join(ROOT, "tools", "phase2verifybench_ref.js"), init_path, pt_path,
                        key_path, "5"], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, NTHREADS=str(threads)))
    if p.returncode != 0:
        raise SystemExit(f"the reference leg failed at 2^{lg}:\n{p.stderr[-2000:]}")
    ref = json.loads(p.stdout.strip().splitlines()[-1])
    ptau = open(pt_path, "rb").read()
    verdicts = [pv.verify_from_init(init, ptau, key)]                 # warm-up: code objects, allocator
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        verdicts.append(pv.verify_from_init(init, ptau, key))
        ts.append(time.perf_counter() - t0)
    row = dict(leg="whole", curve=curve, lg=lg, n_vars=n_vars, zkey_bytes=len(key), device_s=round(statistics.median(ts), 4), device_min_max=[round(min(ts), 4), round(max(ts), 4)],
               reference_s=round(statistics.median(ref["ms"]) / 1e3, 4), reference_min_max=[round(min(ref["ms"]) / 1e3, 4), round(max(ref["ms"]) / 1e3, 4)],
               reference_threads=ref["threads"], verdicts_true=all(v is True for v in verdicts) and all(v is True for v in ref["verdicts"]))
    row["ratio"] = round(row["reference_s"] / row["device_s"], 2)
    for f in (r1_path, pt_path, init_path, key_path):
        os.unlink(f)
    if not row["verdicts_true"]:
        raise SystemExit(f"2^{lg}: a verdict is not true: {json.dumps(row)}")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=20)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--curve", default="bn128")
    ap.add_argument("--whole-min-lg", type=int, default=12)
    ap.add_argument("--whole-max-lg", type=int, default=14)
    ap.add_argument("--threads", type=int, default=16, help="worker threads of the reference leg")
    ap.add_argument("--out")
    a = ap.parse_args()
    zkmi.init()
    rows = []
    for curve in ("bn128", "bls12381"):
        rows.append(generator_leg(curve, a.lg, max(a.reps, 10)))
        print(json.dumps(rows[-1]), flush=True)
    node = shutil.which("node")
    if node is None or not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "build", "snarkjs.min.js")):
        rows.append(dict(leg="whole", not_measured="no node or no staged reference bundle"))
        print(json.dumps(rows[-1]), flush=True)
    else:
        tmp = tempfile.mkdtemp(prefix="phase2verifybench-")
        try:
            for lg in range(a.whole_min_lg, a.whole_max_lg + 1):
                rows.append(whole_leg(a.curve, lg, tmp, node, a.threads))
                print(json.dumps(rows[-1]), flush=True)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        json.dump(dict(tool="phase2verifybench", rows=rows), open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
