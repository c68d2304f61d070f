"""Groth16 phase 2 (zkey contribute): the one-scalar scaling kernel against the general batchApplyKey kernel, and the whole device call against the reference.

    python tools/phase2bench.py [--lg 20] [--reps 12] [--whole-min-lg 12] [--whole-max-lg 14] [--curve bn128] [--threads 16] [--out result.json]

(a) Kernel alone, both curves, n = 2^lg G1 points ((7 * 11^i) G, generated on the device), one random scalar: zkmi_group_scale_dev against
zkmi_group_batch_apply_key_dev(first = k, inc = 1) in the same process, alternating, 2 warm-ups and the median of --reps device times (the events the library
records around its launches: zkmi_last_kernel_ms). The two outputs must be the same bytes.
(b) Whole call, --curve, domains 2^whole-min-lg .. 2^whole-max-lg: a key from tools/setupbench.py's generator (circuit-shaped r1cs, trapdoor ptau, device newZKey), then the
reference's WASM zKey.contribute (tools/phase2bench_ref.js, --threads worker threads) against groth16_phase2.contribute with the 64 random bytes the reference drew;
the bytes are compared at every size. Needs node and the reference bundle staged in oracle/_ref; without them (b) is reported as not measured."""
import argparse
import ctypes as C
import hashlib
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
import oracle_lib as O  # noqa: E402
from snarkjs_amd import groth16_phase2 as p2, groth16_setup as gs, zkmi  # noqa: E402


def kernel_leg(curve, lg, reps):
    cv = next(c for c in gs.CURVES.values() if c["name"] == curve)
    cid, n, L = cv["id"], 1 << lg, zkmi.lib()
    size = n * 2 * cv["n8q"]
    d_in, d_a, d_b = zkmi.DeviceBuffer(size), zkmi.DeviceBuffer(size), zkmi.DeviceBuffer(size)
    zkmi.check(L.zkmi_gen_geometric_bases_dev(cid, 1, n, 7, 11, d_in.ptr))
    k = np.frombuffer((0x1f2e3d4c5b6a79881726354453627180aabbccddeeff00112233445566778899 % cv["r"]).to_bytes(32, "little"), np.uint8).copy()
    one = O.fr_one(cid).copy()

    def scale():
        zkmi.check(L.zkmi_group_scale_dev(cid, 1, d_in.ptr, d_a.ptr, n, zkmi.ptr(k)))
        zkmi.check(L.zkmi_synchronize())
        return L.zkmi_last_kernel_ms()

    def general():
        zkmi.check(L.zkmi_group_batch_apply_key_dev(cid, 1, d_in.ptr, d_b.ptr, n, zkmi.ptr(k), zkmi.ptr(one)))
        zkmi.check(L.zkmi_synchronize())
        return L.zkmi_last_kernel_ms()
    for _ in range(2):
        scale(); general()
    ts, tg = [], []
    for _ in range(reps):
        ts.append(scale()); tg.append(general())
    same = d_a.to_host().tobytes() == d_b.to_host().tobytes()
    for d in (d_in, d_a, d_b):
        d.free()
    row = dict(leg="kernel", curve=curve, lg=lg, reps=reps, group_scale_ms=round(statistics.median(ts), 3), group_scale_min_max=[round(min(ts), 3), round(max(ts), 3)],
               batch_apply_key_ms=round(statistics.median(tg), 3), batch_apply_key_min_max=[round(min(tg), 3), round(max(tg), 3)], same_bytes=same)
    row["ratio"] = round(row["batch_apply_key_ms"] / row["group_scale_ms"], 2)
    return row


def whole_leg(curve, lg, tmp, node, threads):
    import setupbench
    from snarkjs_amd.workloads import synth_r1cs
    r1_path, pt_path, key_path = (os.path.join(tmp, f"c{lg}.{e}") for e in ("r1cs", "ptau", "zkey"))
    data, n_vars = synth_r1cs.circuit_shaped(curve, lg)
    open(r1_path, "wb").write(data)
    setupbench.trapdoor_ptau(curve, lg, pt_path)
    zkey, _cs = gs.new_zkey(r1_path, pt_path)
    open(key_path, "wb").write(zkey)
    p = subprocess.run([node, "--harmony-optional-chaining", "--harmony-nullish", "--max-old-space-size=16384", os.path.join(ROOT, "tools", "phase2bench_ref.js"), key_path, "bench", "Entropy"],
                       capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, NTHREADS=str(threads)))
    if p.returncode != 0:
        raise SystemExit(f"the reference leg failed at 2^{lg}:\n{p.stderr[-2000:]}")
    ref = json.loads(p.stdout.strip().splitlines()[-1])
    rnd = bytes.fromhex(ref["random64"])
    p2.contribute(zkey, "bench", "Entropy", rnd)                      # warm-up: code objects, allocator
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        out, h = p2.contribute(zkey, "bench", "Entropy", rnd)
        ts.append(time.perf_counter() - t0)
    row = dict(leg="whole", curve=curve, lg=lg, n_vars=n_vars, zkey_bytes=len(zkey), device_s=round(statistics.median(ts), 4), reference_s=round(ref["ms"] / 1e3, 4),
               reference_threads=ref["threads"], same_bytes=hashlib.sha256(out).hexdigest() == ref["sha256"] and h.hex() == ref["contributionHash"])
    row["ratio"] = round(row["reference_s"] / row["device_s"], 2)
    for f in (r1_path, pt_path, key_path):
        os.unlink(f)
    if not row["same_bytes"]:
        raise SystemExit(f"2^{lg}: the device key differs from the reference's: {json.dumps(row)}")
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
        rows.append(kernel_leg(curve, a.lg, max(a.reps, 10)))
        print(json.dumps(rows[-1]), flush=True)
    node = shutil.which("node")
    if node is None or not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "build", "snarkjs.min.js")):
        rows.append(dict(leg="whole", not_measured="no node or no staged reference bundle"))
        print(json.dumps(rows[-1]), flush=True)
    else:
        tmp = tempfile.mkdtemp(prefix="phase2bench-")
        try:
            for lg in range(a.whole_min_lg, a.whole_max_lg + 1):
                rows.append(whole_leg(a.curve, lg, tmp, node, a.threads))
                print(json.dumps(rows[-1]), flush=True)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        json.dump(dict(tool="phase2bench", rows=rows), open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
