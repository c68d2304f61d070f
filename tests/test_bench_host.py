"""Host-side logic of bench.py that needs no GPU: the budget guard of other_configs (a config that does not fit what is left of --other-configs-budget / --total-budget is
reported as skipped, never run and never silently dropped) and the per-workload lookup of measured HBM traffic."""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_other_configs_budget_guard(monkeypatch):
    bench = importlib.import_module("bench")
    calls = []
    monkeypatch.setattr("subprocess.run", lambda *a, **k: calls.append(a) or (_ for _ in ()).throw(AssertionError("a child was started")))
    args = argparse.Namespace(other_configs_budget=0.0, total_budget=10_000.0, no_cpu_baseline=False, no_ref_wasm=False)
    res = bench.other_configs(args)
    assert set(res) == {"configs[4]", "configs[3]", "configs[1] on a circuit-shaped key", "configs[2] at N=1"}
    assert all("skipped" in v and "budget" in v["skipped"] for v in res.values()) and not calls
    # the whole-run budget binds too, counted from process start
    args = argparse.Namespace(other_configs_budget=10_000.0, total_budget=0.0, no_cpu_baseline=False, no_ref_wasm=False)
    res = bench.other_configs(args)
    assert all("skipped" in v for v in res.values()) and not calls


def test_pmc_traffic_is_looked_up_per_workload():
    bench = importlib.import_module("bench")
    t = bench.pmc_traffic("groth16:bn128:2^20:b_zero_every=0:uniform", "k_msm_accum29_g2s<Bn254Fq>")     # r06: one Fq2 component per lane
    assert t is not None and 2.0e9 < t < 3.5e9
    assert bench.pmc_traffic("groth16:bls12381:2^20:b_zero_every=0:uniform", "k_msm_accum29_g2s<Bls12381Fq>") > 3.0e9
    assert bench.pmc_traffic("plonk:bn128:2^20:additions=524285", "k_msm_accum29<Bn254Fq>") > 1.0e9
    assert bench.pmc_traffic("groth16:bn128:2^24:b_zero_every=0:uniform", "k_msm_accum29_g2s<Bn254Fq>") > 3.5e10
    # a workload that was never counted gets no figure from another one
    assert bench.pmc_traffic("groth16:bn128:2^16:b_zero_every=0:uniform", "k_msm_accum29_g2s<Bn254Fq>") is None
    assert bench.pmc_traffic("groth16:bn128:2^20:b_zero_every=3:uniform", "k_msm_accum29_g2s<Bn254Fq>") is None


def test_dump_outputs_hold_every_word_exactly(tmp_path):
    """--dump-outputs: field elements go out as float64 32-bit words that give the element back bit for bit; a dump beyond 64 MB is refused"""
    import numpy as np
    import pytest
    bench = importlib.import_module("bench")
    x, y = 21888242871839275222246405745257275088696311157297823662689037894645226208582, 2 ** 253 + 12345
    arrays = bench.proof_arrays({"A": [str(x), str(y), "1"], "eval_a": str(y), "protocol": "plonk", "nested": {"T": [str(x)]}}, ["7"], 32)
    assert set(arrays) == {"A", "eval_a", "nested_T", "public_signals"} and arrays["A"].shape == (3, 8) and arrays["eval_a"].shape == (1, 8)
    bench.dump_outputs(str(tmp_path / "out"), arrays)
    a = np.load(tmp_path / "out" / "A.npy")
    assert a.dtype == np.float64
    assert [int.from_bytes(row.astype("<u4").tobytes(), "little") for row in a] == [x, y, 1]
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros((8 << 20) + 1)})
    assert not (tmp_path / "big").exists()
