"""bench.py as every later change is measured with it: a plain run times --steps iterations and
prints the headline line only; --dump-outputs DIR writes what the timed path computed in its last
step, and those arrays are the ones a caller driving the same chain in-process receives.
"""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

G, P, N, K, THIN, ASM = 8, 50, 200, 10, 5, 4
STEPS, WARMUP = 10, 4


def test_plain_run_and_dumped_outputs(dcfm, tmp_path):
    import bench
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--g", str(G), "--P", str(P), "--nobs", str(N), "--K", str(K), "--asm-batch", str(ASM),
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["metric"] == bench.METRIC and out["unit"] == "iter/s" and out["dtype"] == "f64"
    assert out["higher_is_better"] is True and out["full"] is False
    assert out["steps"] == STEPS and out["warmup"] == WARMUP and out["value"] > 0
    assert out["ms_per_step"] == pytest.approx(1e3 / out["value"], rel=1e-2)
    for leg in ("kernels", "roofline", "ingest", "diagnostics", "sigma_error", "sigma_error_converged",
                "cpu_baseline", "cpu_baseline_faithful"):
        assert leg not in out, leg            # those run only with --full

    # the same chain in-process: warm-up run, then the timed run
    Y = bench.synth_data(N, G * P)
    keep = np.flatnonzero(dcfm.count_nonzero_columns(Y) != 0)
    assert keep.size == G * P
    init = dcfm.driver._HostVarind(1, keep.size)
    smp = dcfm.Sampler(N, P, G, K, 0.5, 0, WARMUP + STEPS, THIN, seed=1, asm_batch=ASM)
    try:
        smp.set_data_raw(Y, dcfm.shard_columns(keep, init.varind, P, 0, G))
        smp.init_state()
        smp.run(1, WARMUP)
        smp.run(WARMUP + 1, STEPS)
        state = smp.get_state()
        S = smp.get_sigma()
    finally:
        smp.close()

    files = {f.stem: np.load(f) for f in out_dir.glob("*.npy")}
    assert set(files) == set(dcfm.STATE_FIELDS) | {"Sigma_cols"}
    assert all(a.dtype == np.float64 for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64_000_000
    for f in dcfm.STATE_FIELDS:
        assert np.array_equal(files[f], state[f]), f
    # Sigma_cols: whole columns of Sigmaout, stripes of 8 adjacent ones
    C = files["Sigma_cols"]
    assert C.shape == (G * P, 32)
    for j in range(0, 32, 8):
        c0 = int(np.flatnonzero((S == C[:, j:j + 1]).all(axis=0))[0])
        assert c0 % 8 == 0 and np.array_equal(C[:, j:j + 8], S[:, c0:c0 + 8])
