"""Writes the r1cs fixtures of the FFLONK setup tests: tests/golden/fflonk_setup_bn128_{quirks,rows30,rows31}.r1cs (snarkjs_amd/workloads/synth_r1cs.py).
tools/gen_fflonk_setup_golden.js runs it as its first step, so the keys are always made from what the generators build now."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from snarkjs_amd.workloads import synth_r1cs  # noqa: E402

FIXTURES = (("quirks", lambda: synth_r1cs.fflonk_quirks_circuit("bn128")), ("rows30", lambda: synth_r1cs.fflonk_rows_circuit("bn128", 30)),
            ("rows31", lambda: synth_r1cs.fflonk_rows_circuit("bn128", 31)))

if __name__ == "__main__":
    for name, make in FIXTURES:
        data = synth_r1cs.write_r1cs("bn128", *make())
        path = os.path.join(ROOT, "tests", "golden", f"fflonk_setup_bn128_{name}.r1cs")
        open(path, "wb").write(data)
        print(path, len(data), "bytes")
