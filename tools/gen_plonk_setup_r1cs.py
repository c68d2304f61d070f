"""Writes the r1cs fixtures of the PLONK setup tests: tests/golden/plonk_setup_<curve>_{mix,tiny}.r1cs (snarkjs_amd/workloads/synth_r1cs.py).
tools/gen_plonk_setup_golden.js runs it as its first step, so the keys are always made from what the generators build now."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from snarkjs_amd.workloads import synth_r1cs  # noqa: E402

for curve in ("bn128", "bls12381"):
    for name, make in (("mix", synth_r1cs.plonk_mix_circuit), ("tiny", synth_r1cs.plonk_tiny_circuit)):
        data = synth_r1cs.write_r1cs(curve, *make(curve))
        path = os.path.join(ROOT, "tests", "golden", f"plonk_setup_{curve}_{name}.r1cs")
        open(path, "wb").write(data)
        print(path, len(data), "bytes")
