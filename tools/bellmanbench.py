"""The Bellman phase-2 round trip: the fused H basis change against the composition of calls it replaces, and the three whole device calls against the reference.

    python tools/bellmanbench.py [--lgs 16,20] [--whole-lgs 12,14,16] [--curve bn128] [--threads 16] [--out result.json]

(a) Kernel alone, --curve, n = 2^lg resident G1 points ((7 * 11^i) G, generated on the device): zkmi_bellman_h_section_dev in both directions against the
composition it replaces on resident buffers, export = zkmi_group_fft_dev + zkmi_group_batch_apply_key_dev(-2, w) + zkmi_group_convert_dev(LEM -> U), import =
zkmi_group_convert_dev(U -> LEM) + zkmi_group_batch_apply_key_dev(-(1/2), 1/w) + zkmi_group_fft_dev(inverse); a warm-up and the median of 5 wall times each
(min .. max kept), each call followed by zkmi_synchronize. The outputs must be the same bytes.
(b) Whole calls, --curve, domains 2^lg: a key from tools/setupbench.py's generator (circuit-shaped r1cs, trapdoor ptau, device newZKey), then the reference's
WASM exportBellman, bellmanContribute and importBellman (tools/bellmanbench_ref.js, --threads worker threads) against the three calls of groth16_bellman with the
64 random bytes the reference drew; the sha256 of all three files is compared at every size. Needs node and the reference bundle staged in oracle/_ref; without
them (b) is reported as not measured. The probes of the box (zkmi_calibrate_box) go on the last line."""
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
from snarkjs_amd import groth16_bellman as gb, groth16_setup as gs, zkmi  # noqa: E402


def med(ts):
    return dict(s=round(statistics.median(ts), 5), min_max=[round(min(ts), 5), round(max(ts), 5)])


def timed(f, reps=5):
    f()                                                              # warm-up: code objects, work buffers
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return ts


def mont(r, v):
    return np.frombuffer((((v % r) << 256) % r).to_bytes(32, "little"), np.uint8).copy()


def kernel_leg(curve, lg):
    cv = next(c for c in gs.CURVES.values() if c["name"] == curve)
    cid, n, L, r = cv["id"], 1 << lg, zkmi.lib(), cv["r"]
    size = n * 2 * cv["n8q"]
    d_in, d_a, d_b, d_t, d_back_a, d_back_b = (zkmi.DeviceBuffer(size) for _ in range(6))
    zkmi.check(L.zkmi_gen_geometric_bases_dev(cid, 1, n, 7, 11, d_in.ptr))
    wb = np.zeros(32, np.uint8)
    zkmi.check(L.zkmi_fr_root(cid, lg + 1, zkmi.ptr(wb)))
    w = int.from_bytes(wb.tobytes(), "little") * pow(1 << 256, -1, r) % r
    k_exp, k_imp = (mont(r, -2), mont(r, w)), (mont(r, -pow(2, -1, r)), mont(r, pow(w, -1, r)))
    sync = lambda: zkmi.check(L.zkmi_synchronize())  # noqa: E731

    def fused(src, dst, direction):
        zkmi.check(L.zkmi_bellman_h_section_dev(cid, src.ptr, dst.ptr, lg, direction)); sync()

    def composed_export():
        zkmi.check(L.zkmi_group_fft_dev(cid, 1, d_in.ptr, d_t.ptr, lg, 0))
        zkmi.check(L.zkmi_group_batch_apply_key_dev(cid, 1, d_t.ptr, d_b.ptr, n, zkmi.ptr(k_exp[0]), zkmi.ptr(k_exp[1])))
        zkmi.check(L.zkmi_group_convert_dev(cid, 1, zkmi.CONV_LEM_TO_U, d_b.ptr, d_t.ptr, n - 1)); sync()      # the last point is dropped: d_t holds the n - 1 H points

    def composed_import():
        zkmi.check(L.zkmi_memset_dev(d_back_b.ptr, 0, size))                                                      # the zero last point
        zkmi.check(L.zkmi_group_convert_dev(cid, 1, zkmi.CONV_U_TO_LEM, d_a.ptr, d_back_b.ptr, n - 1))
        zkmi.check(L.zkmi_group_batch_apply_key_dev(cid, 1, d_back_b.ptr, d_b.ptr, n, zkmi.ptr(k_imp[0]), zkmi.ptr(k_imp[1])))
        zkmi.check(L.zkmi_group_fft_dev(cid, 1, d_b.ptr, d_back_b.ptr, lg, 1)); sync()
    row = dict(leg="kernel", curve=curve, lg=lg)
    row["export_fused"], row["export_composed"] = med(timed(lambda: fused(d_in, d_a, 0))), med(timed(composed_export))
    used = (n - 1) * 2 * cv["n8q"]
    same_e = d_a.to_host()[:used].tobytes() == d_t.to_host()[:used].tobytes()
    row["import_fused"], row["import_composed"] = med(timed(lambda: fused(d_a, d_back_a, 1))), med(timed(composed_import))
    same_i = d_back_a.to_host().tobytes() == d_back_b.to_host().tobytes()
    row["same_bytes"] = same_e and same_i
    row["export_ratio"] = round(row["export_composed"]["s"] / row["export_fused"]["s"], 2)
    row["import_ratio"] = round(row["import_composed"]["s"] / row["import_fused"]["s"], 2)
    for d in (d_in, d_a, d_b, d_t, d_back_a, d_back_b):
        d.free()
    if not row["same_bytes"]:
        raise SystemExit(f"2^{lg}: the fused call and the composition differ: {json.dumps(row)}")
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
    p = subprocess.run([node, "--harmony-optional-chaining", "--harmony-nullish", "--max-old-space-size=16384", os.path.join(ROOT, "tools", "bellmanbench_ref.js"), key_path, curve, "Entropy", "bench"],
                       capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, NTHREADS=str(threads)))
    if p.returncode != 0:
        raise SystemExit(f"the reference leg failed at 2^{lg}:\n{p.stderr[-2000:]}")
    ref = json.loads(p.stdout.strip().splitlines()[-1])
    rnd = bytes.fromhex(ref["random64"])
    ch = gb.export_bellman(zkey)
    rs, h = gb.bellman_contribute(curve, ch, "Entropy", rnd)
    new = gb.import_bellman(zkey, rs, "bench")
    sha = [hashlib.sha256(b).hexdigest() for b in (ch, rs, new)]
    t_e, t_c, t_i = timed(lambda: gb.export_bellman(zkey)), timed(lambda: gb.bellman_contribute(curve, ch, "Entropy", rnd)), timed(lambda: gb.import_bellman(zkey, rs, "bench"))
    row = dict(leg="whole", curve=curve, lg=lg, n_vars=n_vars, zkey_bytes=len(zkey), reference_threads=ref["threads"], same_sha256=sha == ref["sha256"] and h.hex() == ref["contributionHash"])
    for k, ts, ms in (("export", t_e, ref["ms"][0]), ("contribute", t_c, ref["ms"][1]), ("import", t_i, ref["ms"][2])):
        row[k] = dict(device=med(ts), reference_s=round(ms / 1e3, 4), ratio=round(ms / 1e3 / statistics.median(ts), 2))
    for f in (r1_path, pt_path, key_path):
        os.unlink(f)
    if not row["same_sha256"]:
        raise SystemExit(f"2^{lg}: the device files differ from the reference's: {json.dumps(row)}")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lgs", default="16,20")
    ap.add_argument("--whole-lgs", default="12,14,16")
    ap.add_argument("--curve", default="bn128")
    ap.add_argument("--threads", type=int, default=16, help="worker threads of the reference leg")
    ap.add_argument("--out")
    a = ap.parse_args()
    zkmi.init()
    rows = []

    def keep(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        if a.out:
            json.dump(dict(tool="bellmanbench", rows=rows), open(a.out, "w"), indent=1)
    for lg in [int(x) for x in a.lgs.split(",") if x]:
        keep(kernel_leg(a.curve, lg))
    node = shutil.which("node")
    if node is None or not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "build", "snarkjs.min.js")):
        keep(dict(leg="whole", not_measured="no node or no staged reference bundle"))
    else:
        tmp = tempfile.mkdtemp(prefix="bellmanbench-")
        try:
            for lg in [int(x) for x in a.whole_lgs.split(",") if x]:
                keep(whole_leg(a.curve, lg, tmp, node, a.threads))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    x, y = C.c_double(), C.c_double()
    if zkmi.lib().zkmi_calibrate_box(C.byref(x), C.byref(y)) == 0:
        keep(dict(leg="box", mul29_gmul_per_s=round(x.value, 1), gather128_gb_per_s=round(y.value, 1)))


if __name__ == "__main__":
    main()
