"""Writes tests/golden/oracle_flip_levels.json: per oracle-farm case that has an fp32 pass (tests/oracle_farm.py: want32)
and per gradient tensor, how far the oracle's own formulas evaluated in fp32 are from the fp64 oracle on the two
populations of rows the gradient bars distinguish (oracle_farm.flip_sensitive_rows, the fp32 oracle standing in for the side
under test):

    flip_rows, flip_max, flip_median, flip_p90          the flip-sensitive rows: how many, largest error / tensor scale,
                                                        median and 90th percentile of the per-row relative error
    stable_rows, stable_max, stable_median, stable_p90  the same over the decision-stable rows

How far one flipped decision moves a gradient row is a property of the scene, so the largest `flip_max` of this file is the
yardstick for oracle_farm.FLIP_CAP (= min(2e-2, 2 x that figure), derived when oracle_farm is imported).  A sibling of
make_oracle_checksums.py:

    python tests/golden/make_oracle_flip_levels.py [workers]      (about ten minutes on 8 cores; no GPU, no reference import)

Figures are rounded to four digits: the fp32 pass sums in an order that depends on the CPU and the thread count.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "oracle_flip_levels.json")


def levels_of(F, res):
    """The figures of one case from its oracle result (the fp32 oracle is the side under test: its radii are radii32)."""
    import torch
    sens = F.flip_sensitive_rows(res, res["radii32"])
    n = int(sens.numel())
    out = {}
    for k, go in res["grads"].items():
        entry = {}
        for name, rows in (("flip", sens), ("stable", ~sens)):
            st = F.summarize(None, go, n, rows=rows, d=torch.as_tensor(res["d32"][k]))
            entry.update({f"{name}_rows": int(rows.sum()), f"{name}_max": st["normwise"], f"{name}_median": st["median"],
                          f"{name}_p90": st["p90"]})
        out[k] = {m: (v if isinstance(v, int) else float(f"{v:.4g}")) for m, v in entry.items()}
    return out


def main():
    os.environ.setdefault("FARM_WORKERS", sys.argv[1] if len(sys.argv) > 1 else "4")
    os.environ.setdefault("FARM_TORCH_THREADS", "2")
    if not os.path.exists(OUT):          # oracle_farm derives FLIP_CAP from this file when it is imported; this script does not use it
        with open(OUT, "w") as f:
            json.dump({"(first run)": {"-": {"flip_max": 0.0}}}, f)
    import oracle_farm as F
    # importing the test modules registers their cases
    import test_gpu_rasterizer, test_gpu_deep_lists, test_gpu_wide_payload  # noqa: F401
    keys = sorted(k for k, sp in F.FARM.specs.items() if sp["want32"])
    for k in keys:                       # the populations are drawn at the margin the bars use
        F.FARM.specs[k]["sens_tols"] = (1e-3,)
    F.FARM.start(keys)
    out = {}
    for key in keys:
        out[key] = levels_of(F, F.FARM.get(key))
        print(key, {k: f"{v['flip_max']:.3e}/{v['stable_max']:.3e}" for k, v in out[key].items()}, flush=True)
    F.FARM.shutdown()
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    worst = max((t["flip_max"], f"{case} {k}") for case, ts in out.items() for k, t in ts.items())
    print(f"{len(out)} cases written; largest flip-row figure {worst[0]:.4g} ({worst[1]})")


if __name__ == "__main__":
    main()
