"""The three fused Node provers used at the same time in one process (tests/js/concurrent_provers_gpu.js): PLONK, FFLONK and Groth16 proofs started together in
every order, mixed curves, a synchronous prover in the middle of pending proofs, a verify batch alongside, errors that stay local — every proof the reference's own
seeded one — and, where the reference's bundle is staged, the same through registerAll(snarkjs, { fused: true })."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "snarkjs_amd", "napi", "zkmi_napi.node")
NODE = shutil.which("node")
FLAGS = ["--harmony-optional-chaining", "--harmony-nullish"]
need_node = pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")


@pytest.mark.gpu
@need_node
def test_concurrent_provers_of_three_protocols_on_gpu():
    r = subprocess.run([NODE] + FLAGS + [os.path.join(ROOT, "tests", "js", "concurrent_provers_gpu.js")], capture_output=True, text=True, timeout=600)
    sys.stdout.write(r.stdout[-8000:])
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
