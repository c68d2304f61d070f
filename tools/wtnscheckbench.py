"""wtns.check measured; one MI355X, writes profiles/wtnscheckbench.json with --out and the README row with --readme.

Per size (BN254, 2^12, 2^16 and 2^20 constraints by default) one SATISFIABLE heavy-tailed circuit and its witness (snarkjs_amd/workloads/synth_r1cs.py:
satisfiable_circuit with two rows in a thousand of 10^2 - 10^3 terms; written once into --workdir and read from there afterwards, so that making them is not part of any run), and a second witness with
one bad value. Same files, same box, same run; a warm-up and the median of 5 each (min .. max kept):
    (a) reference   tools/wtnscheckbench_ref.js: wtns.check of unmodified snarkjs on the two files
    (b) check       snarkjs_amd.wtns_check.check from the two paths, split into reading the files, the offset pass with upload and layout (zkmi_r1cs_load) and the
                    check (zkmi_r1cs_check)
    (c) resident    Checker.check of one witness on a resident layout, and Checker.check_many of 16
Equal verdicts (good: true, bad: false at the same constraint as the CPU restatement where it is cheap to run) are a condition of every row."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from snarkjs_amd import wtns_check, zkmi  # noqa: E402
from snarkjs_amd.workloads import synth_r1cs as S  # noqa: E402

NODE = ["node", "--harmony-optional-chaining", "--harmony-nullish", "--max-old-space-size=8000"]


def med(ts):
    return round(statistics.median(ts), 5)


def span(ts):
    return [round(min(ts), 5), round(max(ts), 5)]


def timed(fn, reps=5):
    fn()                                                   # warm-up: code objects, allocator, page cache
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def files(workdir, lg):
    """paths of the r1cs, the good and the bad witness of 2^lg constraints, made on first use; -> (paths, index of the constraint the bad witness fails)"""
    os.makedirs(workdir, exist_ok=True)
    stem = os.path.join(workdir, f"wtnscheck_bn128_{lg}")
    paths = (stem + ".r1cs", stem + "_good.wtns", stem + "_bad.wtns", stem + ".json")
    if not all(os.path.exists(p) for p in paths):
        n = 1 << lg
        nv, no, ni, cons, wit = S.satisfiable_circuit("bn128", n, seed=0xbe7c + lg, tail=0.002)
        at = 3 * (n // 4)                                  # a constraint that solves a signal, three quarters of the way down
        bad = list(wit)
        bad[max(s for s, _ in cons[at][2])] += 1
        open(paths[0], "wb").write(S.write_r1cs("bn128", nv, no, ni, cons))
        open(paths[1], "wb").write(S.write_wtns("bn128", wit))
        open(paths[2], "wb").write(S.write_wtns("bn128", bad))
        json.dump(dict(first_bad=at, n_vars=nv, terms=sum(len(lc) for c in cons for lc in c)), open(paths[3], "w"))
    return paths[:3], json.load(open(paths[3]))


def reference(r1cs, wtns, reps, cap):
    r = subprocess.run(NODE + [os.path.join(ROOT, "tools", "wtnscheckbench_ref.js"), r1cs, wtns, str(reps), str(cap)], capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit("reference leg failed:\n" + r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def row(workdir, lg, reps, cap, with_reference):
    (r1cs, good, bad), meta = files(workdir, lg)
    out = dict(curve="bn128", log_n=lg, n_constraints=1 << lg, n_vars=meta["n_vars"], terms=meta["terms"], r1cs_bytes=os.path.getsize(r1cs))
    dev = wtns_check.Device()
    # (b) from paths, and its parts
    t_all = timed(lambda: wtns_check.check(r1cs, good), reps)
    t_read = timed(lambda: (open(r1cs, "rb").read(), open(good, "rb").read()), reps)
    head, handle = wtns_check.read_r1cs(r1cs)
    body = wtns_check._read_body(handle, 2, "r1cs")
    handle[0].close()
    wh, hw = wtns_check.read_wtns_header(good)
    w_good = wtns_check._read_body(hw, 2, "wtns")
    hw[0].close()
    wh, hw = wtns_check.read_wtns_header(bad)
    w_bad = wtns_check._read_body(hw, 2, "wtns")
    hw[0].close()
    keys = []
    t_load = timed(lambda: keys.append(dev.load("bn128", body, head["nConstraints"], head["nVars"])), reps)
    for k in keys[1:]:
        dev.release(k)
    key = keys[0]
    t_check = timed(lambda: dev.check(key, w_good, 1), reps)
    dev.release(key)
    verdict_good, verdict_bad = wtns_check.check(r1cs, good), None
    with wtns_check.Checker(r1cs) as ck:
        t_one = timed(lambda: ck.check(w_good), reps)
        batch = [w_good, w_bad] * 8
        t_16 = timed(lambda: ck.check_many(batch), reps)
        verdict_bad = ck.check_many([w_bad])[0]
        batch_ok = ck.check_many(batch) == [None, meta["first_bad"]] * 8
    if verdict_good is not True or verdict_bad != meta["first_bad"] or not batch_ok:
        raise SystemExit(f"2^{lg}: the device's verdicts are not the expected ones ({verdict_good}, {verdict_bad}, {batch_ok})")
    out.update(check_s=med(t_all), check_min_max=span(t_all), read_s=med(t_read), load_s=med(t_load), load_min_max=span(t_load), device_check_s=med(t_check),
               device_check_min_max=span(t_check), resident_one_s=med(t_one), resident_one_min_max=span(t_one), resident_16_s=med(t_16), resident_16_min_max=span(t_16),
               verdicts=dict(good=True, bad_first=verdict_bad))
    if with_reference:
        ref, ref_bad = reference(r1cs, good, reps, cap), reference(r1cs, bad, 0, cap)
        if ref["verdict"] is not True or ref_bad["verdict"] is not False:
            raise SystemExit(f"2^{lg}: the reference's verdicts differ ({ref['verdict']}, {ref_bad['verdict']})")
        ts = [m / 1e3 for m in ref["ms"]]
        out.update(reference_s=med(ts), reference_min_max=span(ts), reference_capped=ref["capped"], ratio_check=round(med(ts) / med(t_all), 2), ratio_resident=round(med(ts) / med(t_one), 2))
    return out


def readme_row(rows):
    have = [r for r in rows if "reference_s" in r]
    if not have:
        return "**not measured**"
    sizes = " / ".join(f"2^{r['log_n']}" for r in have)
    return ("**" + " / ".join(f"x{r['ratio_check']}" for r in have) + f"** the reference's `wtns.check` on the same files in the same run at {sizes} constraints (from paths "
            + " / ".join(f"{r['check_s']} ({r['check_min_max'][0]} .. {r['check_min_max'][1]})" for r in have) + " s against " + " / ".join(f"{r['reference_s']}" for r in have)
            + " s; one resident witness " + " / ".join(f"{r['resident_one_s']}" for r in have) + " s, 16 in one call " + " / ".join(f"{r['resident_16_s']}" for r in have)
            + " s; BN254, satisfiable heavy-tailed circuits, equal verdicts, one MI355X, one run, median of 5 after a warm-up; `tools/wtnscheckbench.py`)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="12,16,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cap", type=float, default=120.0, help="seconds a reference warm-up may take before it is reported as the one run")
    ap.add_argument("--workdir", default=os.path.join(ROOT, "tools", "bin", "wtnscheckbench"))
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--make-files", action="store_true", help="only write the input files (needs no device)")
    ap.add_argument("--out")
    ap.add_argument("--rows-from", help="take the rows from this result file instead of measuring (with --readme)")
    ap.add_argument("--readme", action="store_true", help="rewrite the README row from the rows measured")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    if a.make_files:
        for lg in sizes:
            print(files(a.workdir, lg)[0][0])
        return
    if a.rows_from:                                         # the README row from a result file written earlier with --out
        rows = json.load(open(a.rows_from))["rows"]
    else:
        zkmi.init()
        rows = []
        for lg in sizes:
            rows.append(row(a.workdir, lg, a.reps, a.cap, not a.no_reference))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
        res = dict(tool="tools/wtnscheckbench.py", device=zkmi.lib().zkmi_version().decode(), reps=a.reps, rows=rows)
        print(json.dumps(res))
        if a.out:
            json.dump(res, open(a.out, "w"), indent=1)
    if a.readme:
        p = os.path.join(ROOT, "README.md")
        lines = open(p).read().split("\n")
        for i, ln in enumerate(lines):
            if "<!-- WTNS-CHECK-ROW -->" in ln:
                cells = ln.split("|")
                cells[2] = " <!-- WTNS-CHECK-ROW -->" + readme_row(rows) + " "
                lines[i] = "|".join(cells)
        open(p, "w").write("\n".join(lines))


if __name__ == "__main__":
    main()
