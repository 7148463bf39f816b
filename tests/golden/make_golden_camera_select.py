"""Writes tests/golden/camera_select.npz from the reference's own CameraClustering (identification/clustering_cameras.py) and,
for the Tanks-and-Temples set, its CameraLoader.  Needs scikit-learn (the reference imports it).

    python tests/golden/make_golden_camera_select.py /path/to/reference

The reference's module is loaded by file path with a stub analyzer that has only `.views`.  Its per-k score and inertia and its
final labels are read from the locals of its own functions while they run.  Per set the file holds the inputs ([N,4,4] world_mat
stack; the tyt pose rows as well) and the reference's best_k, final labels, selected_indices (for tyt also the // 2 mapping),
representative scores, and per k the inertia and the score.

The script refuses to write a set on which a decision hangs on the last bits:
  * for every k, the best fit's inertia must lie at least 1e-6 (relative) below that of every fit with another partition;
  * the winning score and each representative's score must lead the runner-up by at least 1e-9.
(The inertia gaps come from gaussmart_amd.camera_select's per-fit details: scikit-learn keeps only the best fit.)
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from gaussmart_amd import camera_select as CS  # noqa: E402

INERTIA_GAP, SCORE_GAP = 1e-6, 1e-9


def load_reference(root):
    pkg = types.ModuleType("identification")
    pkg.__path__ = []
    stub = types.ModuleType("identification.analyze_cameras")
    stub.AnalyzeCameras = type("AnalyzeCameras", (), {})
    sys.modules.update({"identification": pkg, "identification.analyze_cameras": stub})
    mods = []
    for name in ("clustering_cameras", "camera_loader"):
        spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(root, "identification", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods[0].CameraClustering, mods[1].CameraLoader


def look_at(position, target=np.zeros(3)):
    """c2w whose third column looks from `position` at `target`."""
    z = target - position
    z = z / np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0], z)
    x = x / np.linalg.norm(x)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, np.cross(z, x), z, position
    return c2w


def ring(n, rng):
    a = np.sort(rng.uniform(0, 2 * np.pi, n))
    r = 3.0 + 0.25 * rng.normal(size=n)
    return np.stack([r * np.cos(a), r * np.sin(a), 0.8 + 0.3 * rng.normal(size=n)], 1)


def dome(n, rng):
    v = rng.normal(size=(n, 3))
    v[:, 2] = np.abs(v[:, 2]) + 0.1
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v * (3.0 + 0.3 * rng.normal(size=(n, 1)))


def blob(n, rng):
    return rng.normal(size=(n, 3)) * np.array([2.0, 1.2, 0.6]) + np.array([0.5, -0.3, 2.5])


def grouped_dome(sizes, rng):
    """A dome whose cameras stand in groups of the given sizes, shuffled.  Two cameras alone in a cluster tie EXACTLY in the
    reference's representative score (both are equally far from their mean and share one angle), and its choice between them
    hangs on rounding; with about two cameras per cluster, as at N = 31 with k up to 15, uniform domes always hold such pairs.  So
    the small sets are built from groups of one or of at least three."""
    centres = []
    while len(centres) < len(sizes):
        c = dome(1, rng)[0]
        if all(np.linalg.norm(c - o) > 1.1 for o in centres):
            centres.append(c)
    pos = np.concatenate([c + 0.12 * rng.normal(size=(m, 3)) for c, m in zip(centres, sizes)])
    return pos[rng.permutation(len(pos))]


GROUPS = {"dome31": [3] * 8 + [1] * 7, "dome8": [3, 3, 1, 1], "dome7": [4, 1, 1, 1], "tyt20": [3] * 5 + [1] * 5}


def world_mats(positions, projection=False):
    K = np.array([[2892.3, 0.0, 823.2, 0.0], [0.0, 2883.2, 619.1, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    mats = np.stack([np.linalg.inv(look_at(p)) for p in positions])
    return K @ mats if projection else mats      # DTU: world_mat is the projection K [R|t], which the reference inverts as it stands


# one seed per set, searched so that both margins hold (a cluster of two members ties its two scores exactly, for instance)
SEEDS = {"ring49": 6, "dome64": 10, "dome31": 0, "dome8": 0, "dome7": 0, "blob120": 1, "tyt20": 0}


def build_set(name, seed):
    rng = np.random.default_rng([seed, sum(name.encode())])
    if name == "tyt20":     # Tanks and Temples: 2 x 20 pose rows (3x4 c2w, near, far); the reference's loader keeps the first half
        pos = np.concatenate([grouped_dome(GROUPS[name], rng), dome(20, rng)])
        return np.stack([np.concatenate([look_at(p)[:3, :4].reshape(-1), [0.5, 8.0]]) for p in pos])
    if name in GROUPS:
        return world_mats(grouped_dome(GROUPS[name], rng))
    kind, n = {"r": ring, "d": dome, "b": blob}[name[0]], int(name.lstrip("ringdomeblob"))
    return world_mats(kind(n, rng), projection=name.startswith("ring"))


def build_sets():
    sets = {name: build_set(name, seed) for name, seed in SEEDS.items() if name != "tyt20"}
    sets["tyt20_poses"] = build_set("tyt20", SEEDS["tyt20"])
    return sets


def run_reference(CameraClustering, views):
    rec = {"k": {}}

    def local(frame, event, arg):
        loc = frame.f_locals
        # the line after `score = ...` overwrites what the lines before it recorded under this k (the previous k's score)
        if frame.f_code.co_name == "analyze_optimal_k" and "score" in loc and hasattr(loc["km"], "inertia_"):
            rec["k"][int(loc["k"])] = (float(loc["km"].inertia_), float(loc["score"]))
        if frame.f_code.co_name == "select_representative_cameras" and event == "return":
            rec["labels"], rec["best_k"] = np.asarray(loc["labels"]).copy(), int(loc["k"])
        return local

    def tracer(frame, event, arg):
        return local if frame.f_code.co_name in ("analyze_optimal_k", "select_representative_cameras") else None

    cc = CameraClustering(types.SimpleNamespace(views=views))
    sys.settrace(tracer)
    try:
        res = cc.select_representative_cameras()
    finally:
        sys.settrace(None)
    return res, rec


def check_margins(name, views, res, rec):
    details = {}
    mine = CS.select_representative_cameras(views, details=details)
    for k, (labels, inertia, b) in details["all_fits"].items():
        for f in range(len(inertia)):
            other = not (CS.is_same_clustering(labels[f], labels[b], k) and CS.is_same_clustering(labels[b], labels[f], k))
            if other and not inertia[f] >= inertia[b] * (1 + INERTIA_GAP):
                raise SystemExit(f"{name}: k = {k}: fit {f} ({inertia[f]!r}) is within {INERTIA_GAP} of the best ({inertia[b]!r})")
    scores = sorted((s for _, s in rec["k"].values()), reverse=True)
    if scores[0] - scores[1] < SCORE_GAP:
        raise SystemExit(f"{name}: the two best scores {scores[:2]} are closer than {SCORE_GAP}")
    if min(details["margins"]) < SCORE_GAP:
        raise SystemExit(f"{name}: a representative leads its runner-up by {min(details['margins'])}")
    if mine["selected_indices"] != [int(i) for i in res["selected_indices"]]:
        raise SystemExit(f"{name}: this repository selects {mine['selected_indices']}, the reference {res['selected_indices']}")
    gap = min(inertia[f] / inertia[b] - 1 for labels, inertia, b in details["all_fits"].values() for f in range(len(inertia))
              if not CS.is_same_clustering(labels[f], labels[b], labels.max() + 1) and inertia[b] > 0)
    print(f"{name}: N = {len(views)}, best_k = {rec['best_k']}, selected = {mine['selected_indices']}, smallest inertia gap {gap:.2e}, "
          f"score lead {scores[0] - scores[1]:.2e}, smallest representative lead {min(details['margins']):.2e}")


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    CameraClustering, CameraLoader = load_reference(sys.argv[1])
    sets = build_sets()
    poses = sets.pop("tyt20_poses")
    out = {"sets": np.array(sorted(sets) + ["tyt20"]), "tyt20_poses": poses}
    with tempfile.TemporaryDirectory() as tmp:
        np.save(os.path.join(tmp, "poses_bounds.npy"), poses)
        tyt_views = CameraLoader.load_tyt_cameras(os.path.join(tmp, "poses_bounds.npy"))
    sets["tyt20"] = np.stack([tyt_views[i]["world_mat"] for i in range(len(tyt_views))])
    for name, mats in sets.items():
        views = {i: {"world_mat": m} for i, m in enumerate(mats)}
        res, rec = run_reference(CameraClustering, views)
        check_margins(name, views, res, rec)
        ks = sorted(rec["k"])
        out.update({f"{name}_world_mat": mats, f"{name}_best_k": np.int64(rec["best_k"]), f"{name}_labels": rec["labels"].astype(np.int64),
                    f"{name}_selected": np.array(res["selected_indices"], np.int64), f"{name}_ks": np.array(ks, np.int64),
                    f"{name}_inertia": np.array([rec["k"][k][0] for k in ks]), f"{name}_score": np.array([rec["k"][k][1] for k in ks]),
                    f"{name}_rep_score": np.array([res["cluster_info"][c]["score"] for c in range(rec["best_k"])])})
    out["tyt20_mapped"] = out["tyt20_selected"] // 2
    path = os.path.join(HERE, "camera_select.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
