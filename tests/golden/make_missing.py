"""Writes tests/golden/missing_chain.json: the scores of the reference imputation chains that
tests/test_gpu_missing.py compares the device's chains with.

The reference is oracle.vectorised.gibbs_iteration followed by the imputation step in NumPy
(tests/missing_cases.reference_chain), from the fixed start of missing_cases.chain_case(): 8 chain seeds, per chain
r (RMSE of the posterior mean over the missing entries against the held-back truth, over that of column-mean
imputation) and c (the share of missing entries within 2 sd_total of the truth).  Run from the repository root:

    python tests/golden/make_missing.py
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import missing_cases as mc  # noqa: E402


def main():
    cc = mc.chain_case()
    assert int(cc["mask"].sum()) == mc.CHAIN["nmiss"]
    out = {"settings": {k: (list(v) if isinstance(v, tuple) else v) for k, v in mc.CHAIN.items()}, "r": [], "c": []}
    for seed in mc.CHAIN["seeds"]:
        r, c = mc.reference_chain(cc, seed)
        print(f"seed {seed}: r {r:.4f} c {c:.4f}")
        out["r"].append(r)
        out["c"].append(c)
    (Path(__file__).resolve().parent / "missing_chain.json").write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
