"""Groth16 setup (zkey new), PLONK setup and FFLONK setup: the device path against the reference's WASM newZKey / plonk.setup / fflonk.setup on the
same files, on the same box.

    python tools/setupbench.py [--protocol groth16|plonk|fflonk] [--curve bn128] [--cap-s 120] [--max-lg 20] [--out result.json]

Per size 2^lg: a circuit-shaped r1cs (snarkjs_amd/workloads/synth_r1cs.py: circuit_shaped) and a prepared ptau synthesised from a known trapdoor
(only the slices newZKey reads hold points: the Lagrange levels lg and lg + 1 and the tauG1 powers; the other levels are zero bytes). At the first size
the reference's own newZKey must accept the synthetic ptau and produce the SAME BYTES as the device path, else the tool stops. It starts at 2^12 and
doubles while the reference leg stays under --cap-s seconds (default 120); beyond that, and at 2^20, the device runs alone. Every ratio printed is
reference / device on the same key in the same run. Kernel times per section come from zkmi_groth16_setup_phase_ms. With --protocol plonk the same
files go through snarkjs_amd/plonk_setup.py: setup and the reference's plonk.setup (2^lg is then the size of the r1cs; the PLONK domain is what the gate
lowering makes of it, reported per row as plonk_constraints and domain_lg together with the four phase times of zkmi_plonk_setup_phase_ms: lowering on the
host, sigma, P4, commitments; these are host wall times around a stream synchronisation, one sample each, reported as phase_wall_ms, not kernel times). --protocol fflonk does the same through snarkjs_amd/fflonk_setup.py and fflonk.setup (BN254
only), with a ptau whose first 9 * 2^domain_lg + 18 tauG1 powers are real (fflonk_trapdoor_ptau) and the phases of zkmi_fflonk_setup_phase_ms: lowering on the
host, sigma, P4, C0 and its commitment. Needs a device, node and the reference bundle staged in oracle/_ref (make -C oracle _ref)."""
import argparse
import ctypes as C
import hashlib
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
from snarkjs_amd import fflonk_setup as fs, groth16_setup as gs, plonk_setup as ps, zkmi  # noqa: E402
from snarkjs_amd.workloads import synth_r1cs  # noqa: E402

TRAPDOOR = {"tau": 0x1234567890ABCDEF1234567, "alpha": 0xA1FA0001, "beta": 0xBE7A0002}


def _mont(r, v):
    return np.frombuffer(((v % r) << 256).__mod__(r).to_bytes(32, "little"), np.uint8).copy()


def _points(cid, group, scalars_plain):
    n = scalars_plain.size // 32
    d_s, d_o = zkmi.DeviceBuffer.from_host(scalars_plain), zkmi.DeviceBuffer(n * 2 * group * O.n8q(cid))
    zkmi.check(zkmi.lib().zkmi_gen_bases_from_scalars_dev(cid, group, d_s.ptr, n, d_o.ptr))
    out = d_o.to_host()
    d_s.free(); d_o.free()
    return out


def lagrange_at_tau(cid, r, lg, tau):
    """L_c(tau) for the domain 2^lg, normal form, n x 32 bytes (oracle field vectors)"""
    n = 1 << lg
    one = O.fr_one(cid)
    rep = lambda e, k: np.tile(np.asarray(e, np.uint8), k)
    scale = lambda vec, k: O.apply_key(cid, vec, _mont(r, k), one)
    w = int.from_bytes(O.from_mont(cid, O.fr_w(cid, lg)).tobytes(), "little")
    wp = O.apply_key(cid, rep(one, n), _mont(r, 1), _mont(r, w))
    den = scale(O.vec_op(cid, "sub", rep(_mont(r, tau), n), wp), n)
    return scale(O.vec_op(cid, "mul", wp, O.batch_inverse(cid, den)), (pow(tau, n, r) - 1) % r)      # Montgomery


def trapdoor_ptau(curve, lg, path):
    """a prepared ptau of power lg + 1 in which the slices newZKey reads for a 2^lg domain are real"""
    cv = next(c for c in gs.CURVES.values() if c["name"] == curve)
    q = next(k for k, c in gs.CURVES.items() if c is cv)
    cid, r, power = cv["id"], cv["r"], lg + 1
    s1, s2 = 2 * cv["n8q"], 4 * cv["n8q"]
    tau, alpha, beta = (TRAPDOOR[k] % r for k in ("tau", "alpha", "beta"))
    one = O.fr_one(cid)
    nrm = lambda v: O.from_mont(cid, v)
    rep = lambda e, k: np.tile(np.asarray(e, np.uint8), k)
    n_tau = (2 << power) - 1
    powers = O.apply_key(cid, rep(one, 1 << (lg + 1)), _mont(r, 1), _mont(r, tau))                  # tau^i, i < 2^(lg+1): all newZKey reads
    sec2 = np.zeros(n_tau * s1, np.uint8)
    sec2[:(2 << lg) * s1] = _points(cid, 1, nrm(powers))
    L = lagrange_at_tau(cid, r, lg, tau)
    L2 = lagrange_at_tau(cid, r, lg + 1, tau)
    scale = lambda vec, k: O.apply_key(cid, vec, _mont(r, k), one)

    def lag_section(sz, group, vec, with_next):
        levels = power + (2 if with_next else 1)                       # section 12 also holds the level power + 1 (src/powersoftau_preparephase2.js)
        sec = np.zeros(((1 << levels) - 1) * sz, np.uint8)
        d = 1 << lg
        sec[(d - 1) * sz:(2 * d - 1) * sz] = _points(cid, group, nrm(vec))
        if with_next:
            sec[(2 * d - 1) * sz:(4 * d - 1) * sz] = _points(cid, group, nrm(L2))
        return sec
    sec3 = np.zeros((1 << power) * s2, np.uint8)
    sec3[:2 * s2] = _points(cid, 2, nrm(powers[:64]))                   # [1]_2 and [tau]_2: plonk.setup copies the second one into its header (X_2)
    secs = [(1, struct.pack("<I", cv["n8q"]) + q.to_bytes(cv["n8q"], "little") + struct.pack("<II", power, power)),
            (2, sec2), (3, sec3), (4, _points(cid, 1, nrm(_mont(r, alpha)))), (5, _points(cid, 1, nrm(_mont(r, beta)))),
            (6, _points(cid, 2, nrm(_mont(r, beta)))), (7, struct.pack("<I", 0)),
            (12, lag_section(s1, 1, L, True)), (13, lag_section(s2, 2, L, False)), (14, lag_section(s1, 1, scale(L, alpha), False)), (15, lag_section(s1, 1, scale(L, beta), False))]
    with open(path, "wb") as f:
        f.write(b"ptau" + struct.pack("<II", 1, len(secs)))
        for typ, body in secs:
            body = body.tobytes() if isinstance(body, np.ndarray) else body
            f.write(struct.pack("<IQ", typ, len(body)))
            f.write(body)


def fflonk_trapdoor_ptau(lg, path):
    """a BN254 ptau that holds what fflonk.setup reads for a 2^lg domain: the first 9 * 2^lg + 18 tauG1 powers (all real), [1]_2 and [tau]_2, an empty section 12"""
    cv = next(c for c in gs.CURVES.values() if c["name"] == "bn128")
    q = next(k for k, c in gs.CURVES.items() if c is cv)
    cid, r, n = cv["id"], cv["r"], 9 * (1 << lg) + 18
    tau = TRAPDOOR["tau"] % r
    powers = O.from_mont(cid, O.apply_key(cid, np.tile(np.asarray(O.fr_one(cid), np.uint8), n), _mont(r, 1), _mont(r, tau)))
    secs = [(1, struct.pack("<I", 32) + q.to_bytes(32, "little") + struct.pack("<II", lg + 4, lg + 4)), (2, _points(cid, 1, powers).tobytes()),
            (3, _points(cid, 2, powers[:64]).tobytes()), (12, b"")]
    with open(path, "wb") as f:
        f.write(b"ptau" + struct.pack("<II", 1, len(secs)))
        for typ, body in secs:
            f.write(struct.pack("<IQ", typ, len(body)))
            f.write(body)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--protocol", default="groth16", choices=["groth16", "plonk", "fflonk"])
    ap.add_argument("--curve", default="bn128")
    ap.add_argument("--cap-s", type=float, default=120.0, help="the reference leg stops doubling once one run took longer than this")
    ap.add_argument("--min-lg", type=int, default=12)
    ap.add_argument("--max-lg", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    zkmi.init()
    node = shutil.which("node")
    rows, ref_alive = [], node is not None and os.path.exists(os.path.join(ROOT, "oracle", "_ref", "build", "snarkjs.min.js"))
    if not ref_alive:
        print("no node or no staged reference bundle: device leg only", file=sys.stderr)
    tmp = tempfile.mkdtemp(prefix="setupbench-")
    try:
        sizes = list(range(a.min_lg, a.max_lg + 1))
        for lg in sizes:
            if not ref_alive and lg not in (a.min_lg, a.max_lg):
                continue                                               # past the cap: the device alone at the last size
            r1_path, pt_path = os.path.join(tmp, f"c{lg}.r1cs"), os.path.join(tmp, f"p{lg}.ptau")
            data, n_vars = synth_r1cs.circuit_shaped(a.curve, lg)
            open(r1_path, "wb").write(data)
            plonk, mod = a.protocol != "groth16", fs if a.protocol == "fflonk" else ps          # plonk: either of the two PLONK-style setups
            pt_lg = lg
            if plonk:                                                  # the domain is what the gate lowering makes of the r1cs
                src = gs._Source(data)
                sr = gs.read_sections(src, b"r1cs")
                cv = next(c for c in gs.CURVES.values() if c["name"] == a.curve)
                pt_lg = mod.lower(cv, gs.read_r1cs_header(src, sr), src.read(*sr[2][0]))["domain_size"].bit_length() - 1
            if a.protocol == "fflonk":
                fflonk_trapdoor_ptau(pt_lg, pt_path)
            else:
                trapdoor_ptau(a.curve, pt_lg, pt_path)
            run = (lambda: (mod.setup(r1_path, pt_path), None)) if plonk else (lambda: gs.new_zkey(r1_path, pt_path))
            run()                                                      # warm-up: code objects, allocator
            t0 = time.perf_counter()
            zkey, cs_hash = run()
            dev_s = time.perf_counter() - t0
            ms = (C.c_double * (4 if plonk else 5))()
            L = zkmi.lib()
            zkmi.check((L.zkmi_fflonk_setup_phase_ms if a.protocol == "fflonk" else L.zkmi_plonk_setup_phase_ms if plonk else L.zkmi_groth16_setup_phase_ms)(ms))
            names = ("lowering_host", "sigma", "p4", "c0_commitment" if a.protocol == "fflonk" else "commitments") if plonk else ("A", "B1", "B2", "IC_C", "H")
            row = dict(lg=lg, n_vars=n_vars, r1cs_bytes=len(data), device_s=round(dev_s, 4),
                       **{"phase_wall_ms" if plonk else "kernel_ms": dict(zip(names, [round(x, 3) for x in ms]))},
                       zkey_sha256=hashlib.sha256(zkey).hexdigest())
            if plonk:
                src = gs._Source(zkey)
                o = gs.read_sections(src, b"zkey")[2][0][0] + 4 + gs.CURVES[next(k for k, c in gs.CURVES.items() if c["name"] == a.curve)]["n8q"] + 4 + 32
                _nv, _np, dom, _na, n_pc = struct.unpack_from("<IIIII", zkey, o)
                row.update(plonk_constraints=n_pc, domain_lg=dom.bit_length() - 1, zkey_bytes=len(zkey))
            if ref_alive:
                p = subprocess.run([node, "--harmony-optional-chaining", "--harmony-nullish", "--max-old-space-size=16384", os.path.join(ROOT, "tools", "setupbench_ref.js"), r1_path, pt_path] +
                                   (["--protocol", a.protocol] if plonk else []), capture_output=True, text=True, cwd=ROOT)
                if p.returncode != 0:
                    raise SystemExit(f"the reference leg failed at 2^{lg}:\n{p.stderr[-2000:]}")
                ref = json.loads(p.stdout.strip().splitlines()[-1])
                row.update(reference_s=round(ref["ms"] / 1e3, 4), reference_threads=ref["threads"], same_bytes=ref["sha256"] == row["zkey_sha256"],
                           ratio=round(ref["ms"] / 1e3 / dev_s, 2))
                if not row["same_bytes"] or (not plonk and ref["csHash"] != cs_hash.hex()):
                    raise SystemExit(f"2^{lg}: the device key differs from the reference's on the synthetic files: {json.dumps(row)}")
                if ref["ms"] / 1e3 > a.cap_s:
                    ref_alive = False
            rows.append(row)
            print(json.dumps(row), flush=True)
            os.unlink(r1_path); os.unlink(pt_path)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    res = dict(tool="setupbench", protocol=a.protocol, curve=a.curve, cap_s=a.cap_s, rows=rows)
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
