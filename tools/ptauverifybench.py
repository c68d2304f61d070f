"""powersOfTau.verify: the device driver against the reference's WASM verify on the same prepared BN254 files, on the same box, in the same run.

    python tools/ptauverifybench.py [--min-power 12] [--max-power 14] [--step 2] [--threads 16] [--out result.json]

Per power: unmodified snarkjs with the drop-in makes the file (tools/ptauverifybench_ref.js make: newAccumulator -> contribute -> preparePhase2, not timed as part of
either leg), then the reference's powersOfTau.verify (its own WASM, --threads worker threads, a process of its own) and powersoftau_verify.verify run on that file: a
warm-up and the median of 5 each; both verdicts must be true. The device driver's time is split into reading the file, the four zkmi_ptau_section_check calls, Blake2b on
the host (hashlib: the sections' U form, the first challenge hash, getG2sp), the one zkmi_same_ratio_batch launch and the rest (parsing, hashToG2, conversions of header
points). Needs node and the reference bundle staged in oracle/_ref; without them nothing is measured and the tool says so."""
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
from snarkjs_amd import powersoftau_verify as tv, zkmi  # noqa: E402


class TimedDevice(tv.Device):
    def __init__(self):
        self.t = dict(sections=0.0, same_ratio=0.0)

    def section_check(self, *a):
        t0 = time.perf_counter()
        r = super().section_check(*a)
        self.t["sections"] += time.perf_counter() - t0
        return r

    def same_ratio_batch(self, *a):
        t0 = time.perf_counter()
        r = super().same_ratio_batch(*a)
        self.t["same_ratio"] += time.perf_counter() - t0
        return r


class TimedHashlib:
    """hashlib for the driver, with the time spent in Blake2b added up"""

    def __init__(self):
        self.seconds = 0.0

    def blake2b(self, *a, **k):
        outer, t0 = self, time.perf_counter()
        h = hashlib.blake2b(*a, **k)
        self.seconds += time.perf_counter() - t0

        class H:
            def update(self, b):
                t = time.perf_counter()
                h.update(b)
                outer.seconds += time.perf_counter() - t

            def digest(self):
                t = time.perf_counter()
                d = h.digest()
                outer.seconds += time.perf_counter() - t
                return d
        return H()


def node_json(node, threads, *args):
    p = subprocess.run([node, "--harmony-optional-chaining", "--harmony-nullish", "--max-old-space-size=16384", os.path.join(ROOT, "tools", "ptauverifybench_ref.js")] + list(args),
                       capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, NTHREADS=str(threads)))
    if p.returncode != 0:
        raise SystemExit(f"the reference leg failed ({' '.join(args)}):\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def one_power(power, tmp, node, threads):
    path = os.path.join(tmp, f"p{power}.ptau")
    made = node_json(node, threads, "make", str(power), path)
    ref = node_json(node, threads, "verify", path, "5")
    plain_read, plain_hashlib = tv._Source.read, tv.hashlib
    read_s = [0.0]

    def timed_read(self, off, n):
        t0 = time.perf_counter()
        r = plain_read(self, off, n)
        read_s[0] += time.perf_counter() - t0
        return r
    verdicts, runs = [tv.verify(path)], []                # warm-up: code objects, allocator
    tv._Source.read = timed_read
    try:
        for _ in range(5):
            dev, tv.hashlib, read_s[0] = TimedDevice(), TimedHashlib(), 0.0
            t0 = time.perf_counter()
            verdicts.append(tv._verify(path, None, None, dev))
            total = time.perf_counter() - t0
            runs.append(dict(total=total, read_file=read_s[0], sections=dev.t["sections"], blake2b_host=tv.hashlib.seconds, same_ratio=dev.t["same_ratio"],
                             rest=total - read_s[0] - dev.t["sections"] - tv.hashlib.seconds - dev.t["same_ratio"]))
    finally:
        tv._Source.read, tv.hashlib = plain_read, plain_hashlib
    os.unlink(path)
    med = lambda k: round(statistics.median(r[k] for r in runs), 4)
    ts = [r["total"] for r in runs]
    row = dict(power=power, ptau_bytes=made["bytes"], ceremony_s=round(made["seconds"], 1), made_by=made["made_by"], device_s=med("total"), device_min_max=[round(min(ts), 4), round(max(ts), 4)],
               split_s={k: med(k) for k in ("read_file", "sections", "blake2b_host", "same_ratio", "rest")},
               reference_s=round(statistics.median(ref["ms"]) / 1e3, 4), reference_min_max=[round(min(ref["ms"]) / 1e3, 4), round(max(ref["ms"]) / 1e3, 4)],
               reference_threads=ref["threads"], verdicts_true=all(v is True for v in verdicts) and all(v is True for v in ref["verdicts"]))
    row["ratio"] = round(row["reference_s"] / row["device_s"], 2)
    if not row["verdicts_true"]:
        raise SystemExit(f"2^{power}: a verdict is not true: {json.dumps(row)}")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-power", type=int, default=12)
    ap.add_argument("--max-power", type=int, default=14)
    ap.add_argument("--step", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16, help="worker threads of the reference legs")
    ap.add_argument("--out")
    a = ap.parse_args()
    zkmi.init()
    rows = []
    node = shutil.which("node")
    if node is None or not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "build", "snarkjs.min.js")):
        rows.append(dict(not_measured="no node or no staged reference bundle"))
        print(json.dumps(rows[-1]), flush=True)
    else:
        tmp = tempfile.mkdtemp(prefix="ptauverifybench-")
        try:
            for power in range(a.min_power, a.max_power + 1, a.step):
                rows.append(one_power(power, tmp, node, a.threads))
                print(json.dumps(rows[-1]), flush=True)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        json.dump(dict(tool="ptauverifybench", rows=rows), open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
