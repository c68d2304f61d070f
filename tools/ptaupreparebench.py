"""powersOfTau.preparePhase2: the device driver against the reference on plain WASM and against unmodified snarkjs with the drop-in alone, on the same raw BN254
files, on the same box, in the same run; and the ladder kernels against the loop of single transforms they replace.

    python tools/ptaupreparebench.py [--min-power 8] [--max-power 16] [--step 2] [--threads 16] [--cap-seconds 60] [--ref-max-power 16] [--dropin-max-power 16] [--out result.json] [--append]

Per power: unmodified snarkjs makes the raw file (tools/ptaupreparebench_ref.js make: newAccumulator -> contribute, a process of its own, not timed as part of any
leg), then on that file, a warm-up and the median of 5 each:
    (a) reference_s   the reference's preparePhase2 on plain WASM, --threads worker threads, a process of its own
    (b) dropin_s      unmodified snarkjs with registerAll(snarkjs) alone: one G.ifft on the device per power and section
    (c) device_s      powersoftau_prepare.prepare_phase2, split into reading the file, the four zkmi_ptau_lagrange_section calls and the rest
All three must give the same bytes (sha256). A reference leg whose warm-up run takes longer than --cap-seconds is measured by that one run and marked capped; above
--ref-max-power leg (a), above --dropin-max-power leg (b) is not run at all and the row says so.
Second table (rows "kernels"), for one resident section at powers 12 and 16 and each group, the first 2^power points of section 2 / 3 of that file:
zkmi_ptau_lagrange_dev(first = 0, top = power) against the loop for p = 0 .. power: zkmi_group_fft_dev(prefix, p, inverse) into the same layout, equal bytes, wall time
around a drained stream, a warm-up and the median of 5 each; with the counts of launches and lanes of both.
Needs node and the reference bundle staged in oracle/_ref; without them nothing is measured and the tool says so."""
import argparse
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from snarkjs_amd import powersoftau_prepare as tp, zkmi  # noqa: E402
from snarkjs_amd.groth16_setup import _Source, read_sections  # noqa: E402

BN128 = 0


class TimedDevice(tp.Device):
    def __init__(self):
        self.seconds = 0.0

    def lagrange_section(self, *a):
        t0 = time.perf_counter()
        r = super().lagrange_section(*a)
        self.seconds += time.perf_counter() - t0
        return r


def node_json(node, threads, *args):
    p = subprocess.run([node, "--harmony-optional-chaining", "--harmony-nullish", "--max-old-space-size=16384", os.path.join(ROOT, "tools", "ptaupreparebench_ref.js")] + list(args),
                       capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, NTHREADS=str(threads)))
    if p.returncode != 0:
        raise SystemExit(f"the reference leg failed ({' '.join(args)}):\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def timed(fn, reps=5):
    fn()                                                   # warm-up: code objects, allocator, twiddle tables
    ts = []
    for _ in range(reps):
        zkmi.check(zkmi.lib().zkmi_synchronize())
        t0 = time.perf_counter()
        fn()
        zkmi.check(zkmi.lib().zkmi_synchronize())
        ts.append(time.perf_counter() - t0)
    return ts


def kernel_rows(path, power):
    """the ladder against the loop of single transforms, on one resident section per group"""
    L, rows = zkmi.lib(), []
    src = _Source(path)
    try:
        sections = read_sections(src, b"ptau", 1)
        for group, sec in ((1, 2), (2, 3)):
            sg, n = 64 * group, 1 << power
            tau = src.read(sections[sec][0][0], n * sg)
            n_out = (2 * n - 1) * sg
            d_tau, d_a, d_b = zkmi.DeviceBuffer.from_host(tau), zkmi.DeviceBuffer(n_out), zkmi.DeviceBuffer(n_out)
            try:
                def ladder():
                    zkmi.check(L.zkmi_ptau_lagrange_dev(BN128, group, d_tau.ptr, n, d_a.ptr, 0, power, 0))

                def loop():
                    for p in range(power + 1):
                        zkmi.check(L.zkmi_group_fft_dev(BN128, group, d_tau.ptr, d_b.ptr + ((1 << p) - 1) * sg, p, 1))
                t_ladder, t_loop = timed(ladder), timed(loop)
                same = bool((d_a.to_host() == d_b.to_host()).all())
            finally:
                d_tau.free(); d_a.free(); d_b.free()
            if not same:
                raise SystemExit(f"2^{power} G{group}: the ladder and the loop of single transforms differ")
            med = lambda ts: round(statistics.median(ts), 5)
            # the loop: per power p a load, p stages of 2^(p-1) lanes and a store of 2^p lanes; the ladder: one load and one store of 2^(top+1) - 1 lanes, top stages of 2^top lanes
            rows.append(dict(kernels=True, power=power, group=group, ladder_s=med(t_ladder), ladder_min_max=[round(min(t_ladder), 5), round(max(t_ladder), 5)],
                             loop_s=med(t_loop), loop_min_max=[round(min(t_loop), 5), round(max(t_loop), 5)], ratio=round(med(t_loop) / med(t_ladder), 2), equal_bytes=same,
                             ladder_launches=power + 2, loop_launches=sum(p + 2 for p in range(power + 1)),
                             ladder_stage_lanes=power << power, loop_stage_lanes=sum(p << (p - 1) for p in range(1, power + 1)),
                             butterflies=sum(p << (p - 1) for p in range(1, power + 1))))
    finally:
        src.close()
    return rows


def one_power(power, tmp, node, a):
    path = os.path.join(tmp, f"p{power}_raw.ptau")
    made = node_json(node, a.threads, "make", str(power), path)
    row = dict(power=power, raw_bytes=made["bytes"], ceremony_s=round(made["seconds"], 1), made_by=made["made_by"])
    first = tp.prepare_phase2(path)                         # warm-up
    sha, runs = hashlib.sha256(first).hexdigest(), []
    plain_read, read_s = _Source.read, [0.0]

    def timed_read(self, off, n):
        t0 = time.perf_counter()
        r = plain_read(self, off, n)
        read_s[0] += time.perf_counter() - t0
        return r
    _Source.read = timed_read
    try:
        for _ in range(5):
            dev, read_s[0] = TimedDevice(), 0.0
            t0 = time.perf_counter()
            out = tp._prepare_phase2(path, None, None, dev)
            total = time.perf_counter() - t0
            if out != first:
                raise SystemExit(f"2^{power}: two device runs gave different bytes")
            runs.append(dict(total=total, read_file=read_s[0], sections=dev.seconds, rest=total - read_s[0] - dev.seconds))
    finally:
        _Source.read = plain_read
    med = lambda k: round(statistics.median(r[k] for r in runs), 4)
    ts = [r["total"] for r in runs]
    row.update(prepared_bytes=len(first), device_s=med("total"), device_min_max=[round(min(ts), 4), round(max(ts), 4)], split_s={k: med(k) for k in ("read_file", "sections", "rest")})
    same = True
    for key, mode, limit in (("reference", "plain", a.ref_max_power), ("dropin", "dropin", a.dropin_max_power)):
        if power > limit:
            row[key + "_not_run"] = f"above power {limit}"
            continue
        r = node_json(node, a.threads, "prepare", path, "5", mode, str(a.cap_seconds))
        s = [m / 1e3 for m in r["ms"]]
        row.update({key + "_s": round(statistics.median(s), 4), key + "_min_max": [round(min(s), 4), round(max(s), 4)], key + "_runs": len(s), key + "_capped": r["capped"],
                    "ratio_" + key: round(statistics.median(s) / row["device_s"], 2)})
        row["reference_threads"] = r["threads"]
        same = same and r["sha256"] == sha
    row["same_bytes"] = same
    if not same:
        raise SystemExit(f"2^{power}: the three legs gave different bytes: {json.dumps(row)}")
    rows = [row]
    if power in (12, 16):
        rows += kernel_rows(path, power)
    os.unlink(path)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-power", type=int, default=8)
    ap.add_argument("--max-power", type=int, default=16)
    ap.add_argument("--step", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16, help="worker threads of the reference legs")
    ap.add_argument("--cap-seconds", type=float, default=60.0, help="a reference leg whose warm-up run takes longer is measured by that one run")
    ap.add_argument("--ref-max-power", type=int, default=16, help="leg (a) is not run above this power")
    ap.add_argument("--dropin-max-power", type=int, default=16, help="leg (b) is not run above this power")
    ap.add_argument("--out")
    ap.add_argument("--append", action="store_true", help="keep the rows --out already holds")
    a = ap.parse_args()
    zkmi.init()
    rows = json.load(open(a.out))["rows"] if a.append and a.out and os.path.exists(a.out) else []
    node = shutil.which("node")
    if node is None or not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "build", "snarkjs.min.js")):
        rows.append(dict(not_measured="no node or no staged reference bundle"))
        print(json.dumps(rows[-1]), flush=True)
    else:
        tmp = tempfile.mkdtemp(prefix="ptaupreparebench-")
        try:
            for power in range(a.min_power, a.max_power + 1, a.step):
                for r in one_power(power, tmp, node, a):
                    rows.append(r)
                    print(json.dumps(r), flush=True)
                if a.out:
                    json.dump(dict(tool="ptaupreparebench", rows=rows), open(a.out, "w"), indent=1)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        json.dump(dict(tool="ptaupreparebench", rows=rows), open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
