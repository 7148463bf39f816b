"""Writes tests/golden/adam_bars.json: how far plain fp32 torch is from the float64 reference of tests/adam_ref.py on exactly
the inputs of the optimiser cases (tests/test_gpu_optimizer_edges.py), per quantity and on the scales of the checkers:

    m, v, p       dense step: torch.optim.Adam(foreach=False), one step from the case's state
    m_sh, v_sh    factored SH step: the gradient sum over the views in plain fp32 torch, then the same optimiser
                  (its parameter error goes into p)
    rgb, J        colour cache: sh_basis, its autograd derivative and the sums in fp32, from the fp32 coefficients the
                  restated step wrote

`levels` is the worst figure of each quantity over all cases, `groups` the same per case group.  tests/adam_ref.py turns
the levels into bars (4 x) when it is imported.  The script also checks that the clamp band of the colour cases is as
empty as the checker demands (adam_ref.check_cache asserts it).  A sibling of make_oracle_flip_levels.py:

    python tests/golden/make_adam_bars.py        (a minute on one core; no GPU)

Figures are rounded to four digits.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "adam_bars.json")


def main():
    if not os.path.exists(OUT):          # adam_ref derives its bars from this file when it is imported
        with open(OUT, "w") as f:
            json.dump({"levels": {q: 1.0 for q in ("m", "v", "p", "m_sh", "v_sh", "rgb", "J")}}, f)
    import torch
    import adam_ref as A
    torch.set_num_threads(1)
    inf = float("inf")
    A.BARS.update({q: inf for q in A.QUANTITIES})        # measure: nothing is asserted against a bar of an earlier run
    groups = {}

    def note(group, errs):
        g = groups.setdefault(group, {})
        for q, e in errs.items():
            if q in A.QUANTITIES:
                g[q] = max(g.get(q, 0.0), e)

    for c in A.dense_bar_cases():
        new = A.torch_adam_step(c.p, c.g, c.m, c.v, c.lr, c.t, c.betas, c.eps)
        note("dense " + c.name.split("-")[0], A.check_dense((c.p, c.m, c.v), new, c.g, c.lr, c.t, c.betas, c.eps))
    for c in A.factored_bar_cases():
        new = A.torch_factored_step(c)
        note(f"factored M{c.M}", A.check_factored(c, (c.p, c.m, c.v), new))
    cache_runs = []
    for c in A.cache_bar_cases():
        new = A.torch_factored_step(c)
        note(f"cache M{c.M}", A.check_factored(c, (c.p, c.m, c.v), new))
        col = A.colour_cache(new[0], c.xyz_next, c.campos_next, c.deg_next, dtype=torch.float32)
        cache_runs.append((c, new[0], A.pack_cache(col)))
        note(f"cache M{c.M}", A.cache_errors(cache_runs[-1][2], new[0], c.xyz_next, c.campos_next, c.deg_next)[0])
    levels = {q: max(g.get(q, 0.0) for g in groups.values()) for q in A.QUANTITIES}
    # the band of the clamp comparison at the bar these levels give: as empty as check_cache demands, bits equal outside
    A.BARS.update({q: A.MARGIN * float(f"{levels[q]:.4g}") for q in A.QUANTITIES})
    band = 0
    for c, sh_new, cache in cache_runs:
        band += A.check_cache(cache, sh_new, c.xyz_next, c.campos_next, c.deg_next, exact_rows=c.exact_rows, what=c.name)["band"]
    out = {"levels": {q: float(f"{levels[q]:.4g}") for q in A.QUANTITIES},
           "groups": {k: {q: float(f"{e:.4g}") for q, e in sorted(g.items())} for k, g in sorted(groups.items())},
           "margin": A.MARGIN, "clamp_entries_in_band": band}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for q in A.QUANTITIES:
        print(f"{q:5s} level {out['levels'][q]:.4g}  bar {A.MARGIN * out['levels'][q]:.4g}")


if __name__ == "__main__":
    main()
