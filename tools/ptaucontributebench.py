"""powersOfTau.contribute: the device driver against the reference on plain WASM and against unmodified snarkjs with the drop-in alone, on the same fresh BN254
accumulator with the same random64, on the same box, in the same run; and the per-lane-scalar G1 kernel against the general kernel it stands beside.

    python tools/ptaucontributebench.py [--powers 8,12,16] [--threads 16] [--cap-seconds 60] [--ref-max-power 16] [--dropin-max-power 16] [--kernel-logs 16,20] [--leg-timeout 600] [--out result.json]

Table 1, per power, a warm-up and the median of 5 each (min .. max kept):
    (a) reference_s   the reference's contribute on plain WASM, --threads worker threads, a process of its own (tools/ptaucontributebench_ref.js)
    (b) dropin_s      unmodified snarkjs with registerAll(snarkjs) alone: G.batchApplyKey and the conversions on the device chunk by chunk
    (c) device_s      powersoftau_contribute.contribute on the accumulator new_accumulator made, split into reading the file, the four section calls (with the G2
                      call's share of them), Blake2b on the host (partial state, response and challenge hashes) and the rest; the conversions' share of the section
                      calls is measured beside them: the two zkmi_group_convert_dev launches per section on resident points, drained
All three must give the same bytes (sha256). A reference leg whose warm-up run takes longer than --cap-seconds is measured by that one run and marked capped; a leg
above its --*-max-power, or without node / the staged bundle, is written as "not measured".
Table 2 (rows "kernel"), per curve at 2^16 and 2^20 resident G1 points P_i = (7 * 11^i) G with the scalars first * inc^i in normal form on the device:
zkmi_diag_group_mul_each_dev against zkmi_group_batch_apply_key_dev(first, inc), equal bytes, wall time around a drained stream, a warm-up and the median of 5 each.
`keeps` states the rule of DESIGN.md 20: the new kernel's median below the general kernel's by more than the two min .. max spreads."""
import argparse
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from snarkjs_amd import powersoftau_contribute as tc, zkmi  # noqa: E402
from snarkjs_amd.groth16_setup import CURVES, _Source  # noqa: E402

RANDOM64 = bytes(range(64))
FIRST, INC = 0x1234567890abcdef1234567890abcdef, 0xfedcba0987654321fedcba0987654321


def med(ts):
    return round(statistics.median(ts), 5)


def span(ts):
    return [round(min(ts), 5), round(max(ts), 5)]


def timed(fn, reps=5):
    fn()                                                   # warm-up: code objects, allocator
    ts = []
    for _ in range(reps):
        zkmi.check(zkmi.lib().zkmi_synchronize())
        t0 = time.perf_counter()
        fn()
        zkmi.check(zkmi.lib().zkmi_synchronize())
        ts.append(time.perf_counter() - t0)
    return ts


def kernel_row(cv, log_n):
    L, c, n = zkmi.lib(), cv["id"], 1 << log_n
    sg, r = 2 * cv["n8q"], cv["r"]
    mont = lambda v: np.frombuffer((v % r * (1 << 256) % r).to_bytes(32, "little"), np.uint8).copy()
    first, inc = mont(FIRST), mont(INC)
    ones = np.tile(mont(1), n)
    d_pts, d_k, d_a, d_b = zkmi.DeviceBuffer(n * sg), zkmi.DeviceBuffer.from_host(ones), zkmi.DeviceBuffer(n * sg), zkmi.DeviceBuffer(n * sg)
    try:
        zkmi.check(L.zkmi_gen_geometric_bases_dev(c, 1, n, 7, 11, d_pts.ptr))
        zkmi.check(L.zkmi_fr_batch_apply_key_dev(c, d_k.ptr, d_k.ptr, n, zkmi.ptr(first), zkmi.ptr(inc)))
        zkmi.check(L.zkmi_fr_batch_dev(c, 1, d_k.ptr, d_k.ptr, n))
        t_new = timed(lambda: zkmi.check(L.zkmi_diag_group_mul_each_dev(c, 1, d_pts.ptr, d_k.ptr, d_a.ptr, n)))
        t_old = timed(lambda: zkmi.check(L.zkmi_group_batch_apply_key_dev(c, 1, d_pts.ptr, d_b.ptr, n, zkmi.ptr(first), zkmi.ptr(inc))))
        same = bool((d_a.to_host() == d_b.to_host()).all())
    finally:
        d_pts.free(); d_k.free(); d_a.free(); d_b.free()
    if not same:
        raise SystemExit(f"{cv['name']} 2^{log_n}: the two kernels differ")
    spreads = (max(t_new) - min(t_new)) + (max(t_old) - min(t_old))
    return dict(kernel=True, curve=cv["name"], log_n=log_n, mul_each_s=med(t_new), mul_each_min_max=span(t_new), general_s=med(t_old), general_min_max=span(t_old),
                ratio=round(med(t_old) / med(t_new), 2), equal_bytes=same, keeps=bool(med(t_old) - med(t_new) > spreads))


class TimedDevice(tc.Device):
    def __init__(self):
        self.seconds, self.g2_seconds, self.shapes = 0.0, 0.0, []

    def contribute_section(self, cv, group, body, n, first, inc):
        t0 = time.perf_counter()
        r = super().contribute_section(cv, group, body, n, first, inc)
        dt = time.perf_counter() - t0
        self.seconds += dt
        if group == 2:
            self.g2_seconds += dt
        self.shapes.append((group, n, r[0]))
        return r


def conversions_seconds(cv, shapes):
    """the two conversions of every section on resident points, drained: their share of the section calls' device time"""
    L, total = zkmi.lib(), []
    for group, n, lem in shapes:
        d_lem, d_out = zkmi.DeviceBuffer.from_host(np.frombuffer(lem, np.uint8)), zkmi.DeviceBuffer(len(lem))
        try:
            def both():
                zkmi.check(L.zkmi_group_convert_dev(cv["id"], group, zkmi.CONV_LEM_TO_C, d_lem.ptr, d_out.ptr, n))
                zkmi.check(L.zkmi_group_convert_dev(cv["id"], group, zkmi.CONV_LEM_TO_U, d_lem.ptr, d_out.ptr, n))
            total.append(statistics.median(timed(both)))
        finally:
            d_lem.free(); d_out.free()
    return sum(total)


def node_json(node, threads, timeout, *args):
    """one reference leg in a process of its own, ended (subprocess.TimeoutExpired) after `timeout` seconds: the 'dropin' leg opens the device"""
    p = subprocess.run([node, "--harmony-optional-chaining", "--harmony-nullish", "--max-old-space-size=16384", os.path.join(ROOT, "tools", "ptaucontributebench_ref.js")] + list(args),
                       capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, NTHREADS=str(threads)), timeout=timeout)
    if p.returncode != 0:
        raise SystemExit(f"the reference leg failed ({' '.join(args)}):\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def one_power(power, node, a):
    cv = next(c for c in CURVES.values() if c["name"] == "bn128")
    fresh = tc.new_accumulator("bn128", power)[0]
    first = tc.contribute(fresh, "bench", "Entropy", None, None, RANDOM64)[0]      # warm-up
    sha, runs = hashlib.sha256(first).hexdigest(), []
    plain_read, read_s = _Source.read, [0.0]
    plain_partial, plain_blake, hash_s = tc.blake2b_partial, tc.hashlib.blake2b, [0.0]

    def timed_read(self, off, n):
        t0 = time.perf_counter()
        r = plain_read(self, off, n)
        read_s[0] += time.perf_counter() - t0
        return r

    def timed_partial(chunks):
        t0 = time.perf_counter()
        r = plain_partial(chunks)
        hash_s[0] += time.perf_counter() - t0
        return r

    class TimedBlake:
        def __init__(self, *x, **k):
            t0 = time.perf_counter()
            self.h = plain_blake(*x, **k)
            hash_s[0] += time.perf_counter() - t0

        def update(self, d):
            t0 = time.perf_counter()
            self.h.update(d)
            hash_s[0] += time.perf_counter() - t0

        def digest(self):
            return self.h.digest()

    class HashlibShim:
        blake2b = TimedBlake
        sha256 = hashlib.sha256
    _Source.read, tc.blake2b_partial, tc.hashlib = timed_read, timed_partial, HashlibShim
    try:
        for _ in range(5):
            dev, read_s[0], hash_s[0] = TimedDevice(), 0.0, 0.0
            t0 = time.perf_counter()
            out = tc._contribute(fresh, "bench", "Entropy", None, None, RANDOM64, dev)[0]
            total = time.perf_counter() - t0
            if out != first:
                raise SystemExit(f"2^{power}: two device runs gave different bytes")
            runs.append(dict(total=total, read_file=read_s[0], sections=dev.seconds, sections_g2=dev.g2_seconds, blake2b_host=hash_s[0],
                             rest=total - read_s[0] - dev.seconds - hash_s[0]))
    finally:
        _Source.read, tc.blake2b_partial, tc.hashlib = plain_read, plain_partial, hashlib
    m = lambda k: round(statistics.median(r[k] for r in runs), 4)
    ts = [r["total"] for r in runs]
    row = dict(power=power, fresh_bytes=len(fresh), bytes=len(first), sha256=sha, device_s=m("total"), device_min_max=span(ts),
               split_s={k: m(k) for k in ("read_file", "sections", "sections_g2", "blake2b_host", "rest")},
               conversions_dev_s=round(conversions_seconds(cv, dev.shapes), 5))
    same = True
    for key, mode, limit in (("reference", "plain", a.ref_max_power), ("dropin", "dropin", a.dropin_max_power)):
        if node is None or power > limit:
            row[key + "_s"] = "not measured"
            row[key + "_not_run"] = "no node or no staged reference bundle" if node is None else f"above power {limit}"
            continue
        r = node_json(node, a.threads, a.leg_timeout, str(power), "5", mode, str(a.cap_seconds), RANDOM64.hex())
        s = [x / 1e3 for x in r["ms"]]
        row.update({key + "_s": round(statistics.median(s), 4), key + "_min_max": span(s), key + "_runs": len(s), key + "_capped": r["capped"],
                    "ratio_" + key: round(statistics.median(s) / row["device_s"], 2)})
        row["reference_threads"] = r["threads"]
        same = same and r["sha256"] == sha
    row["same_bytes"] = same
    if not same:
        raise SystemExit(f"2^{power}: the legs gave different bytes: {json.dumps(row)}")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--powers", default="8,12,16")
    ap.add_argument("--threads", type=int, default=16, help="worker threads of the reference legs")
    ap.add_argument("--cap-seconds", type=float, default=60.0, help="a reference leg whose warm-up run takes longer is measured by that one run")
    ap.add_argument("--ref-max-power", type=int, default=16, help="leg (a) is not run above this power")
    ap.add_argument("--dropin-max-power", type=int, default=16, help="leg (b) is not run above this power")
    ap.add_argument("--leg-timeout", type=float, default=600.0, help="a reference leg's process is ended after this many seconds")
    ap.add_argument("--kernel-logs", default="16,20")
    ap.add_argument("--out")
    a = ap.parse_args()
    zkmi.init()
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)
        if a.out:
            json.dump(dict(tool="ptaucontributebench", rows=rows), open(a.out, "w"), indent=1)
    for log_n in [int(x) for x in a.kernel_logs.split(",") if x]:
        for cv in CURVES.values():
            emit(kernel_row(cv, log_n))
    node = shutil.which("node")
    if node is not None and not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "build", "snarkjs.min.js")):
        node = None
    for power in [int(x) for x in a.powers.split(",") if x]:
        emit(one_power(power, node, a))


if __name__ == "__main__":
    main()
