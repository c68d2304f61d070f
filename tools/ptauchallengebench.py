"""The challenge / response round trip measured; one MI355X, writes profiles/ptauchallengebench.json with --out.

Table 2, the kernel alone: zkmi_diag_group2_mul_each_dev against zkmi_group_batch_apply_key_dev(first, inc) on the same resident G2 points (7 * 11^i) G2 with the
scalars first * inc^i, equal bytes, wall time around a drained stream, a warm-up and the median of 5 each (min .. max kept). `keeps` states the rule of
DESIGN.md 21: the new kernel's median below the general kernel's by more than the two min .. max spreads.

Table 1, per power, one challengeContribute on the SAME challenge file (exported here from a fresh BN254 accumulator) with the same random64, a warm-up and the
median of 5 each (min .. max kept):
    (c) device     snarkjs_amd.powersoftau_challenge.challenge_contribute from the file's path, split into reading the file, the five section calls (with the share
                   of the two G2 calls), Blake2b on the host and the rest
    (a) reference  tools/ptauchallengebench_ref.js plain: the reference's WASM with --threads worker threads
    (b) dropin     the same with registerAll(snarkjs) alone, what the parent commit can do
The sha256 of the response must be equal across the legs. Section rows: the five zkmi_ptau_challenge_section calls alone on synthetic points."""
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from snarkjs_amd import powersoftau_challenge as tch, powersoftau_contribute as tc, zkmi  # noqa: E402
from snarkjs_amd.groth16_setup import CURVES  # noqa: E402

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


def mont(cv, v):
    r = cv["r"]
    return np.frombuffer((v % r * (1 << 256) % r).to_bytes(32, "little"), np.uint8).copy()


def kernel_row(cv, log_n):
    L, c, n = zkmi.lib(), cv["id"], 1 << log_n
    sg = 4 * cv["n8q"]
    first, inc = mont(cv, FIRST), mont(cv, INC)
    ones = np.tile(mont(cv, 1), n)
    d_pts, d_k, d_a, d_b = zkmi.DeviceBuffer(n * sg), zkmi.DeviceBuffer.from_host(ones), zkmi.DeviceBuffer(n * sg), zkmi.DeviceBuffer(n * sg)
    try:
        zkmi.check(L.zkmi_gen_geometric_bases_dev(c, 2, n, 7, 11, d_pts.ptr))
        zkmi.check(L.zkmi_fr_batch_apply_key_dev(c, d_k.ptr, d_k.ptr, n, zkmi.ptr(first), zkmi.ptr(inc)))
        zkmi.check(L.zkmi_fr_batch_dev(c, 1, d_k.ptr, d_k.ptr, n))
        t_new = timed(lambda: zkmi.check(L.zkmi_diag_group2_mul_each_dev(c, d_pts.ptr, d_k.ptr, d_a.ptr, n)))
        t_old = timed(lambda: zkmi.check(L.zkmi_group_batch_apply_key_dev(c, 2, d_pts.ptr, d_b.ptr, n, zkmi.ptr(first), zkmi.ptr(inc))))
        same = bool((d_a.to_host() == d_b.to_host()).all())
    finally:
        d_pts.free(); d_k.free(); d_a.free(); d_b.free()
    if not same:
        raise SystemExit(f"{cv['name']} 2^{log_n}: the two kernels differ")
    spreads = (max(t_new) - min(t_new)) + (max(t_old) - min(t_old))
    return dict(kernel=True, curve=cv["name"], log_n=log_n, mul_each_s=med(t_new), mul_each_min_max=span(t_new), general_s=med(t_old), general_min_max=span(t_old),
                ratio=round(med(t_old) / med(t_new), 2), equal_bytes=same, keeps=bool(med(t_old) - med(t_new) > spreads))


def section_row(cv, power):
    """the five section calls of one response on (7 * 11^i) G points in U form"""
    import ctypes as C
    L, c = zkmi.lib(), cv["id"]
    one, tau, alpha, beta = mont(cv, 1), mont(cv, INC), mont(cv, FIRST), mont(cv, FIRST + 2)
    shapes = [(1, (2 << power) - 1, one, tau), (2, 1 << power, one, tau), (1, 1 << power, alpha, tau), (1, 1 << power, beta, tau), (2, 1, beta, tau)]
    bodies = []
    for group, n, _, _ in shapes:
        sg = 2 * group * cv["n8q"]
        d = zkmi.DeviceBuffer(n * sg)
        u = np.zeros(n * sg, np.uint8)
        try:
            zkmi.check(L.zkmi_gen_geometric_bases_dev(c, group, n, 7, 11, d.ptr))
            lem = d.to_host()
        finally:
            d.free()
        zkmi.check(L.zkmi_group_convert(c, group, zkmi.CONV_LEM_TO_U, zkmi.pages_of(lem).pages, (C.c_void_p * 1)(u.ctypes.data), (C.c_size_t * 1)(u.size), 1, n))
        bodies.append((u, np.zeros(n * sg // 2, np.uint8)))

    def call(k):
        group, n, first, inc = shapes[k]
        u, out = bodies[k]
        zkmi.check(L.zkmi_ptau_challenge_section(c, group, zkmi.pages_of(u).pages, n, zkmi.ptr(first), zkmi.ptr(inc), (C.c_void_p * 1)(out.ctypes.data), (C.c_size_t * 1)(out.size), 1, 0))
    t_all = timed(lambda: [call(k) for k in range(5)])
    t_g2 = timed(lambda: [call(k) for k in (1, 4)])
    return dict(sections=True, curve=cv["name"], power=power, five_calls_s=med(t_all), five_calls_min_max=span(t_all), g2_calls_s=med(t_g2), g2_calls_min_max=span(t_g2))


class TimedDevice(tch.Device):
    def __init__(self):
        self.seconds, self.g2_seconds = 0.0, 0.0

    def challenge_section(self, cv, group, body_u, n, first, inc):
        t0 = time.perf_counter()
        r = super().challenge_section(cv, group, body_u, n, first, inc)
        dt = time.perf_counter() - t0
        self.seconds += dt
        if group == 2:
            self.g2_seconds += dt
        return r


def node_json(node, threads, timeout, *args):
    """one reference leg in a process of its own, ended (subprocess.TimeoutExpired) after `timeout` seconds: the 'dropin' leg opens the device"""
    p = subprocess.run([node, "--harmony-optional-chaining", "--harmony-nullish", "--max-old-space-size=16384", os.path.join(ROOT, "tools", "ptauchallengebench_ref.js")] + list(args),
                       capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, NTHREADS=str(threads)), timeout=timeout)
    if p.returncode != 0:
        raise SystemExit(f"the reference leg failed ({' '.join(args)}):\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def one_power(power, node, a, tmp):
    challenge = tch.export_challenge(tc.new_accumulator("bn128", power)[0])[0]
    path = os.path.join(tmp, f"challenge_{power}")
    with open(path, "wb") as f:
        f.write(challenge)
    first = tch.challenge_contribute("bn128", path, None, "Entropy", None, RANDOM64)[0]      # warm-up
    sha, runs = hashlib.sha256(first).hexdigest(), []
    plain_bytes_of, read_s, hash_s = tch._bytes_of, [0.0], [0.0]

    def timed_bytes_of(x):
        t0 = time.perf_counter()
        r = plain_bytes_of(x)
        read_s[0] += time.perf_counter() - t0
        return r

    class TimedBlake:
        def __init__(self, *x, **k):
            t0 = time.perf_counter()
            self.h = hashlib.blake2b(*x, **k)
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
    tch._bytes_of, tch.hashlib, tc.hashlib = timed_bytes_of, HashlibShim, HashlibShim
    try:
        for _ in range(5):
            dev, read_s[0], hash_s[0] = TimedDevice(), 0.0, 0.0
            t0 = time.perf_counter()
            out = tch._challenge_contribute("bn128", path, None, "Entropy", None, RANDOM64, dev)[0]
            total = time.perf_counter() - t0
            if out != first:
                raise SystemExit(f"2^{power}: two device runs gave different bytes")
            runs.append(dict(total=total, read_file=read_s[0], sections=dev.seconds, sections_g2=dev.g2_seconds, blake2b_host=hash_s[0], rest=total - read_s[0] - dev.seconds - hash_s[0]))
    finally:
        tch._bytes_of, tch.hashlib, tc.hashlib = plain_bytes_of, hashlib, hashlib
    m = lambda k: round(statistics.median(r[k] for r in runs), 4)
    ts = [r["total"] for r in runs]
    row = dict(table1=True, power=power, challenge_bytes=len(challenge), bytes=len(first), sha256=sha, device_s=m("total"), device_min_max=span(ts),
               split_s={k: m(k) for k in ("read_file", "sections", "sections_g2", "blake2b_host", "rest")})
    same = True
    for key, mode, limit in (("reference", "plain", a.ref_max_power), ("dropin", "dropin", a.dropin_max_power)):
        if node is None or power > limit:
            row[key + "_s"] = "not measured"
            row[key + "_not_run"] = "no node or no staged reference bundle" if node is None else f"above power {limit}"
            continue
        r = node_json(node, a.threads, a.leg_timeout, path, "5", mode, str(a.cap_seconds), RANDOM64.hex())
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
    ap.add_argument("--kernel-logs", default="16,20")
    ap.add_argument("--threads", type=int, default=16, help="worker threads of the reference legs")
    ap.add_argument("--cap-seconds", type=float, default=60.0, help="a reference leg whose warm-up run takes longer is measured by that one run")
    ap.add_argument("--ref-max-power", type=int, default=16, help="leg (a) is not run above this power")
    ap.add_argument("--dropin-max-power", type=int, default=16, help="leg (b) is not run above this power")
    ap.add_argument("--leg-timeout", type=float, default=600.0, help="a reference leg's process is ended after this many seconds")
    ap.add_argument("--out")
    a = ap.parse_args()
    zkmi.init()
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)
        if a.out:
            json.dump(dict(tool="ptauchallengebench", rows=rows), open(a.out, "w"), indent=1)
    for log_n in [int(x) for x in a.kernel_logs.split(",") if x]:
        for cv in CURVES.values():
            emit(kernel_row(cv, log_n))
    node = shutil.which("node")
    if node is not None and not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "build", "snarkjs.min.js")):
        node = None
    with tempfile.TemporaryDirectory() as tmp:
        for power in [int(x) for x in a.powers.split(",") if x]:
            emit(one_power(power, node, a, tmp))
    for power in [int(x) for x in a.powers.split(",") if x]:
        emit(section_row(next(cv for cv in CURVES.values() if cv["name"] == "bn128"), power))


if __name__ == "__main__":
    main()
