"""Writes the r1cs fixtures of the Groth16 setup tests: tests/golden/setup_<curve>_{edge,full}.r1cs (snarkjs_amd/workloads/synth_r1cs.py).
Run before tools/gen_setup_golden.js:  python tools/gen_setup_r1cs.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from snarkjs_amd.workloads import synth_r1cs  # noqa: E402

for curve in ("bn128", "bls12381"):
    for name, make in (("edge", synth_r1cs.edge_circuit), ("full", synth_r1cs.full_circuit)):
        data = synth_r1cs.write_r1cs(curve, *make(curve))
        path = os.path.join(ROOT, "tests", "golden", f"setup_{curve}_{name}.r1cs")
        open(path, "wb").write(data)
        print(path, len(data), "bytes")
