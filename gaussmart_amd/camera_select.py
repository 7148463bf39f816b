"""Step 1 of the reference's identification/main.py: which views get segmented, and in which order.

identification/clustering_cameras.py runs scikit-learn's KMeans over the normalised camera centres for every k from 3 to 15
(n_init = 10, random_state = 42), scores coverage against compactness, refits at the winning k and takes one representative
camera per cluster, in label order.  Here, decision for decision:

  * the initial centres of ALL fits are drawn on the host from scikit-learn's random stream (kmeans_pp_init: one
    RandomState(42) per k, the ten initialisations in sequence; Lloyd draws nothing);
  * the Lloyd iterations of all 10 (max_k - 2) fits are ONE launch of gsr_cam_lloyd (csrc/cam_cluster.hip, rule CK_LLOYD of
    include/gsr.h), one workgroup per fit, and one read-back; lloyd_batch_host is its numpy twin, equal bit for bit;
  * the best fit per k, the scores and the representative choice are numpy fp64 on the host: their arccos would not round alike
    on the device and they cost microseconds.  The refit at the winning k is the same computation, so its result is reused.

device=None runs the twin.  A k above GSR_CK_KMAX or more cameras than GSR_CK_MAX_CAMERAS run the twin as well.  A fit in which a
cluster loses all members (status 1) is redone on the host with scikit-learn's relocation rule.  scikit-learn is not imported.
"""
import os

import numpy as np

from ._lib import GSR_CK_CHUNK, GSR_CK_KMAX, GSR_CK_MAX_CAMERAS

NERF_IMG_WH = (1024, 1024)          # identification/camera_loader.py:63
TYT_IMG_WH = (979, 543)             # :125
TYT_FOCAL = (501.0, 277.0)          # :127
MIN_K, MAX_K, N_INIT, SEED, MAX_ITER, TOL = 3, 15, 10, 42, 300, 1e-4     # clustering_cameras.py:53-60 and KMeans' defaults
KINDS = ("dtu", "nerf", "tyt")


# ---------------------------------------------------------------- cameras
def _intrinsics(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx, 0.0], [0.0, fy, cy, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])


def load_cameras(path, kind):
    """{view index: camera dict} in the layouts of identification/camera_loader.py."""
    if kind == "dtu":
        views = {}
        with np.load(path) as z:
            for key in z.files:
                name, _, idx = key.rpartition("_")
                if name and idx.isdigit():
                    views.setdefault(int(idx), {})[name] = z[key]
        for i, cam in views.items():
            missing = [k for k in ("world_mat", "camera_mat", "scale_mat") if k not in cam]
            if missing:
                raise ValueError(f"{path}: view {i} lacks {', '.join(missing)}")
        return views
    data = np.load(path)
    if data.ndim != 2:
        raise ValueError(f"{path}: expected a 2-D array of poses, got shape {list(data.shape)}")
    if kind == "nerf":
        if data.shape[1] not in (17, 19):
            raise ValueError(f"{path}: a nerf pose row has 17 or 19 values, got {data.shape[1]}")
        w, h = NERF_IMG_WH
        return {i: {"world_mat": np.linalg.inv(row[:16].reshape(4, 4)), "scale_mat": np.eye(4),
                    "camera_mat": _intrinsics(float(row[16]), float(row[16]), w / 2.0, h / 2.0)} for i, row in enumerate(data)}
    if data.shape[1] not in (14, 16):
        raise ValueError(f"{path}: a tyt pose row has 14 or 16 values, got {data.shape[1]}")
    w, h = TYT_IMG_WH
    views = {}
    for i, row in enumerate(data[:data.shape[0] // 2]):
        c2w = np.eye(4)
        c2w[:3, :4] = row[:12].reshape(3, 4)
        views[i] = {"world_mat": np.linalg.inv(c2w), "scale_mat": np.eye(4), "img_size": np.array([w, h]),
                    "camera_mat": _intrinsics(TYT_FOCAL[0], TYT_FOCAL[1], w / 2.0, h / 2.0)}
    return views


def camera_centres_dirs(views):
    """(positions [N,3], directions [N,3]) in the dict's own order (clustering_cameras.py:27-42): c2w = view['c2w'], else the
    inverse of view['world_mat'] AS IT STANDS (for DTU that is the 4x4 projection K [R|t]); position c2w[:3,3], direction
    c2w[:3,2].  The reference indexes views[idx] with positions in this order, so keys other than 0 .. N-1 ascending are refused."""
    keys = list(views.keys())
    if keys != list(range(len(keys))):
        raise ValueError(f"camera_centres_dirs: the view keys must be 0 .. {len(keys) - 1} in ascending order, got {keys[:8]}"
                         f"{' ...' if len(keys) > 8 else ''}: the selected positions would not index the views")
    pos, dirs = [], []
    for key, view in views.items():
        if "c2w" in view:
            c2w = np.asarray(view["c2w"], np.float64)
        elif "world_mat" in view:
            c2w = np.linalg.inv(np.asarray(view["world_mat"], np.float64))
        else:
            raise ValueError(f"camera_centres_dirs: view {key} has neither c2w nor world_mat")
        pos.append(c2w[:3, 3])
        dirs.append(c2w[:3, 2])
    if not pos:
        return np.empty((0, 3)), np.empty((0, 3))
    return np.vstack(pos), np.vstack(dirs)


def normalize_positions(positions):
    """(normalised, centre, scale): minus the mean, over the per-axis population standard deviation (below 1e-6: 1)."""
    positions = np.asarray(positions, np.float64)
    centre = positions.mean(axis=0)
    centred = positions - centre
    scale = np.std(centred, axis=0)
    scale = np.where(scale < 1e-6, 1.0, scale)
    return centred / scale, centre, scale


# ---------------------------------------------------------------- k-means++ on scikit-learn's random stream
def _sq_distances(A, X, x_sq):
    """scikit-learn's expanded form, so that the candidates round as they do there: -2 A X^T + |A|^2 + |X|^2, floored at 0."""
    d = -2 * (A @ X.T)
    d += np.einsum("ij,ij->i", A, A)[:, None]
    d += x_sq[None, :]
    np.maximum(d, 0, out=d)
    return d


def kmeans_pp_init(X, k, rs):
    """scikit-learn 1.7's _kmeans_plusplus with unit weights on the CENTRED points X [N,3], drawing from the RandomState rs
    what it draws: one choice for the first centre, then per centre 2 + int(log k) uniforms.  -> centres [k,3]."""
    X = np.ascontiguousarray(X, np.float64)
    n = X.shape[0]
    weight = np.ones(n)
    x_sq = np.einsum("ij,ij->i", X, X)
    trials = 2 + int(np.log(k))
    centres = np.empty((k, 3))
    centres[0] = X[rs.choice(n, p=weight / weight.sum())]
    closest = _sq_distances(centres[0, None], X, x_sq)
    pot = closest @ weight
    for c in range(1, k):
        rand = rs.uniform(size=trials) * pot
        ids = np.searchsorted(np.cumsum(weight * closest, dtype=np.float64), rand)
        np.clip(ids, None, closest.size - 1, out=ids)
        dist = _sq_distances(X[ids], X, x_sq)
        np.minimum(closest, dist, out=dist)
        pots = dist @ weight.reshape(-1, 1)
        best = int(np.argmin(pots))
        pot, closest = pots[best], dist[best]
        centres[c] = X[ids[best]]
    return centres


# ---------------------------------------------------------------- CK_LLOYD: the numpy twin and the kernel
def _sqdist(X, C):
    """CK_LLOYD's distance of every point to every row of C: the three squares summed left to right.  [N,len(C)]"""
    d0 = X[:, 0, None] - C[None, :, 0]
    d1 = X[:, 1, None] - C[None, :, 1]
    d2 = X[:, 2, None] - C[None, :, 2]
    return (d0 * d0 + d1 * d1) + d2 * d2


def _ordered(values):
    """The sum from +0 in ascending order, along axis 0."""
    acc = np.zeros(values.shape[1:])
    for v in values:
        acc = acc + v
    return acc


def _lloyd_one(X, centres, k, tol, max_iter, relocate):
    """One fit of CK_LLOYD -> (labels, centres [k,3], inertia, n_iter, status).  np.bincount adds its weights in index order
    from +0, which is the rule's order inside a chunk.  relocate: scikit-learn's answer to an empty cluster instead of status 1."""
    n = len(X)
    chunk = np.arange(n) // GSR_CK_CHUNK
    nchunks = int(chunk[-1]) + 1
    C = np.array(centres[:k], np.float64)
    old = np.full(n, -1, np.int64)
    n_iter, status, relabel = 0, 0, True
    for it in range(max_iter):
        labels = np.argmin(_sqdist(X, C), axis=1)
        n_iter = it + 1
        cell = chunk * k + labels
        sums = np.stack([_ordered(np.bincount(cell, weights=X[:, a], minlength=nchunks * k).reshape(nchunks, k)) for a in range(3)], 1)
        count = _ordered(np.bincount(cell, minlength=nchunks * k).astype(np.float64).reshape(nchunks, k))
        if (count == 0).any():
            if not relocate:
                old, status, relabel = labels, 1, False
                break
            sums, count = _relocate(X, C, sums, count, labels)
        with np.errstate(invalid="ignore", divide="ignore"):
            fresh = np.where(count[:, None] > 0, sums / count[:, None], sums)
        d = fresh - C
        shift = _ordered((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        C = fresh
        same = np.array_equal(labels, old)
        old = labels
        if same:
            relabel = False
            break
        if shift <= tol:
            break
    labels = np.argmin(_sqdist(X, C), axis=1) if relabel else old
    own = X - C[labels]
    d = (own[:, 0] * own[:, 0] + own[:, 1] * own[:, 1]) + own[:, 2] * own[:, 2]
    inertia = float(_ordered(_ordered_chunks(d, chunk, nchunks)))
    return labels.astype(np.int32), C, inertia, n_iter, status


def _ordered_chunks(d, chunk, nchunks):
    return np.bincount(chunk, weights=d, minlength=nchunks)


def _relocate(X, C, sums, count, labels):
    """scikit-learn's _relocate_empty_clusters_dense on the sums: each empty cluster takes the point farthest from its centre."""
    empty = np.where(count == 0)[0]
    dist = ((X - C[labels]) ** 2).sum(axis=1)
    if dist.max() == 0:
        return sums, count
    far = np.argpartition(dist, -len(empty))[:-len(empty) - 1:-1]
    sums, count = sums.copy(), count.copy()
    for new, i in zip(empty, far):
        sums[labels[i]] -= X[i]
        sums[new] = X[i]
        count[new] = 1.0
        count[labels[i]] -= 1.0
    return sums, count


def _batch_args(X, centres0, ks):
    X = np.ascontiguousarray(X, np.float64)
    ks = np.ascontiguousarray(ks, np.int32).reshape(-1)
    centres0 = np.ascontiguousarray(centres0, np.float64)
    if X.ndim != 2 or X.shape[1] != 3 or len(X) < 1:
        raise ValueError(f"lloyd_batch: X must be [N,3] with N >= 1, got {list(X.shape)}")
    if centres0.shape != (len(ks), GSR_CK_KMAX, 3):
        raise ValueError(f"lloyd_batch: centres0 must be [{len(ks)},{GSR_CK_KMAX},3], got {list(centres0.shape)}")
    return X, centres0, ks


def lloyd_batch_host(X, centres0, ks, tol, max_iter=MAX_ITER, relocate=False):
    """CK_LLOYD in numpy, fit by fit: X [N,3] centred, centres0 [F,GSR_CK_KMAX,3], ks [F] -> dict(labels i32 [F,N], centres
    [F,GSR_CK_KMAX,3], inertia [F], n_iter i32 [F], status i32 [F]), the kernel's outputs bit for bit."""
    X, centres0, ks = _batch_args(X, centres0, ks)
    F, n = len(ks), len(X)
    out = dict(labels=np.full((F, n), -1, np.int32), centres=np.zeros((F, GSR_CK_KMAX, 3)), inertia=np.zeros(F),
               n_iter=np.zeros(F, np.int32), status=np.zeros(F, np.int32))
    for f, k in enumerate(ks.tolist()):
        if not 1 <= k <= GSR_CK_KMAX:
            out["status"][f] = 2
            continue
        labels, C, out["inertia"][f], out["n_iter"][f], out["status"][f] = _lloyd_one(X, centres0[f], k, float(tol), int(max_iter), relocate)
        out["labels"][f], out["centres"][f, :k] = labels, C
    return out


def lloyd_batch(X, centres0, ks, tol, max_iter=MAX_ITER, device=None):
    """CK_LLOYD on the device: every fit in one launch of gsr_cam_lloyd and one read-back.  Arguments and result as
    lloyd_batch_host.  More than GSR_CK_MAX_CAMERAS points are refused by the library (the host route is lloyd_batch_host)."""
    import torch
    from . import _dev, _lib
    if device is None:
        raise _lib.GsrError("lloyd_batch: needs device= (no CPU path; see lloyd_batch_host)")
    X, centres0, ks = _batch_args(X, centres0, ks)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.GsrError("lloyd_batch: needs a HIP device (torch 'cuda'); there is no CPU path (see lloyd_batch_host)")
    L = _lib.lib()
    F, n = len(ks), len(X)
    # one upload, one download: [x | centres0] as f64 and k as i32; [centres | inertia] as f64 and [labels | n_iter | status] as i32
    f_in = torch.from_numpy(np.concatenate([X.reshape(-1), centres0.reshape(-1)])).to(dev)
    k_in = torch.from_numpy(ks).to(dev)
    f_out = torch.empty(F * (GSR_CK_KMAX * 3 + 1), dtype=torch.float64, device=dev)
    i_out = torch.empty(F * (n + 2), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        nbytes = L.gsr_cam_lloyd_workspace_bytes(n, F)
        ws = _dev.workspace(nbytes, dev)
        _lib.check(L.gsr_cam_lloyd(_dev.ptr(f_in), n, _dev.ptr(f_in[3 * n:]), _dev.ptr(k_in), F, float(tol), int(max_iter),
                                   _dev.ptr(i_out), _dev.ptr(f_out), _dev.ptr(f_out[F * GSR_CK_KMAX * 3:]), _dev.ptr(i_out[F * n:]),
                                   _dev.ptr(i_out[F * (n + 1):]), _dev.ptr(ws), nbytes, _dev.stream(dev)))
    fo, io = f_out.cpu().numpy(), i_out.cpu().numpy()
    return dict(labels=io[:F * n].reshape(F, n).copy(), centres=fo[:F * GSR_CK_KMAX * 3].reshape(F, GSR_CK_KMAX, 3).copy(),
                inertia=fo[F * GSR_CK_KMAX * 3:].copy(), n_iter=io[F * n:F * (n + 1)].copy(), status=io[F * (n + 1):].copy())


# ---------------------------------------------------------------- KMeans(n_init=10, random_state=42), many k at once
def is_same_clustering(labels1, labels2, k):
    """scikit-learn's _is_same_clustering: every cluster of labels1 lies inside one cluster of labels2."""
    mapping = np.full(k, -1, np.int64)
    for a, b in zip(np.asarray(labels1).tolist(), np.asarray(labels2).tolist()):
        if mapping[a] == -1:
            mapping[a] = b
        elif mapping[a] != b:
            return False
    return True


def pick_best(labels, inertia, k):
    """KMeans.fit's choice among its initialisations: the first fit stands; a later one replaces it only with a strictly lower
    inertia AND another partition.  -> its index."""
    best = 0
    for f in range(1, len(inertia)):
        if inertia[f] < inertia[best] and not is_same_clustering(labels[f], labels[best], k):
            best = f
    return best


def _use_device(device, n, ks):
    return device is not None and n <= GSR_CK_MAX_CAMERAS and max(ks) <= GSR_CK_KMAX


def kmeans_many(X, ks, n_init=N_INIT, seed=SEED, device=None, max_iter=MAX_ITER, tol=TOL, details=None):
    """KMeans(n_clusters=k, n_init=n_init, random_state=seed).fit(X) for every k of ks: {k: (labels [N], centres [k,3],
    inertia)}.  All initialisations of all k are drawn first, then every fit runs in one lloyd_batch (device) or in
    lloyd_batch_host; fits that lost a cluster are redone on the host with scikit-learn's relocation.  details: a dict that
    receives `all_fits`, {k: (labels [n_init,N], inertia [n_init], index of the best)}."""
    X = np.ascontiguousarray(X, np.float64)
    ks = [int(k) for k in ks]
    n = len(X)
    if not ks:
        return {}
    if min(ks) < 1 or max(ks) > n:
        raise ValueError(f"kmeans: k must lie in 1 .. N = {n}, got {min(ks)} .. {max(ks)}")
    tol_abs = float(np.mean(np.var(X, axis=0)) * tol)        # KMeans' _tolerance, on X as it came
    mean = X.mean(axis=0)
    Xc = X - mean
    kmax = max(GSR_CK_KMAX, max(ks))
    centres0 = np.zeros((len(ks) * n_init, kmax, 3))
    fit_k = np.repeat(np.asarray(ks, np.int32), n_init)
    for j, k in enumerate(ks):
        rs = np.random.RandomState(seed)
        for i in range(n_init):
            centres0[j * n_init + i, :k] = kmeans_pp_init(Xc, k, rs)
    if _use_device(device, n, ks):
        res = lloyd_batch(Xc, centres0, fit_k, tol_abs, max_iter, device=device)
    elif kmax > GSR_CK_KMAX:
        res = _wide_host(Xc, centres0, fit_k, tol_abs, max_iter)
    else:
        res = lloyd_batch_host(Xc, centres0, fit_k, tol_abs, max_iter)
    out = {}
    for j, k in enumerate(ks):
        sl = slice(j * n_init, (j + 1) * n_init)
        labels, centres, inertia = res["labels"][sl].copy(), res["centres"][sl].copy(), res["inertia"][sl].copy()
        for i in np.where(res["status"][sl] == 1)[0]:
            labels[i], centres[i, :k], inertia[i], _, _ = _lloyd_one(Xc, centres0[j * n_init + i], k, tol_abs, max_iter, relocate=True)
        b = pick_best(labels, inertia, k)
        out[k] = (labels[b].astype(np.int64), centres[b, :k] + mean, float(inertia[b]))
        if details is not None:
            details.setdefault("all_fits", {})[k] = (labels, inertia, b)
    return out


def _wide_host(Xc, centres0, fit_k, tol_abs, max_iter):
    """The twin for a k above GSR_CK_KMAX (max_cameras given by hand): the same rule, wider centre rows."""
    F, n, kmax = len(fit_k), len(Xc), centres0.shape[1]
    res = dict(labels=np.zeros((F, n), np.int32), centres=np.zeros((F, kmax, 3)), inertia=np.zeros(F), n_iter=np.zeros(F, np.int32),
               status=np.zeros(F, np.int32))
    for f, k in enumerate(fit_k.tolist()):
        res["labels"][f], C, res["inertia"][f], res["n_iter"][f], res["status"][f] = _lloyd_one(Xc, centres0[f], k, tol_abs, max_iter, False)
        res["centres"][f, :k] = C
    return res


def kmeans(X, k, n_init=N_INIT, seed=SEED, device=None):
    """(labels [N], centres [k,3], inertia) of KMeans(n_clusters=k, n_init=n_init, random_state=seed).fit(X)."""
    return kmeans_many(X, [k], n_init, seed, device)[int(k)]


# ---------------------------------------------------------------- the reference's scores (numpy fp64, host)
def _angles_deg(dirs):
    norms = np.linalg.norm(dirs, axis=1, keepdims=True)
    unit = dirs / np.maximum(norms, 1e-8)
    return np.degrees(np.arccos(np.clip(unit @ unit.T, -1.0, 1.0)))


def coverage(positions, directions, labels, k):
    """clustering_cameras.py:62-78 on the UN-normalised positions: per cluster the mean per-axis standard deviation plus the mean
    pairwise angle in degrees / 180 (a lone member: 0 and 90); the sum over k."""
    cov = 0.0
    for c in range(k):
        idx = np.where(labels == c)[0]
        if len(idx) < 1:
            continue
        if len(idx) > 1:
            spread = float(np.mean(np.std(positions[idx], axis=0)))
            ang = float(np.mean(_angles_deg(directions[idx])[np.triu_indices(len(idx), k=1)]))
        else:
            spread, ang = 0.0, 90.0
        cov += spread + ang / 180.0
    return cov / k


def _k_range(n, min_k, max_k):
    if n < 4:
        raise ValueError(f"camera clustering needs at least 4 cameras, got {n} (the reference fails inside scikit-learn there); "
                         "select all views instead (--skip_camera_clustering)")
    max_k = max_k or min(MAX_K, max(min_k + 1, n // 2))
    if min_k < 1 or max_k < min_k or max_k > n:
        raise ValueError(f"camera clustering: k = {min_k} .. {max_k} does not fit {n} cameras")
    return list(range(min_k, max_k + 1))


def analyze_optimal_k(positions, directions, min_k=MIN_K, max_k=None, device=None, details=None):
    """clustering_cameras.py:53-85: the k of the first strictly larger 0.4 coverage + 0.6 compactness.  details: a dict that
    receives `fits` ({k: (labels, centres, inertia)}), `scores` and `inertia` per k."""
    positions, directions = np.asarray(positions, np.float64), np.asarray(directions, np.float64)
    ks = _k_range(len(positions), min_k, max_k)
    X_norm, _, _ = normalize_positions(positions)
    fits = kmeans_many(X_norm, ks, device=device, details=details)
    best_score, best_k, scores = -np.inf, min_k, {}
    for k in ks:
        labels, _, inertia = fits[k]
        compact = -inertia / (np.linalg.norm(X_norm) + 1e-8)
        scores[k] = 0.4 * coverage(positions, directions, labels, k) + 0.6 * compact
        if scores[k] > best_score:
            best_score, best_k = scores[k], k
    if details is not None:
        details.update(fits=fits, scores=scores, inertia={k: fits[k][2] for k in ks})
    return best_k


def select_representative_cameras(views, min_cameras=MIN_K, max_cameras=None, device=None, details=None):
    """clustering_cameras.py:87-140 -> {'selected_indices': [...], 'cluster_info': {c: members, selected, score}}: per cluster,
    in label order, the first camera with the largest 0.5 / (1 + distance to the cluster's world centre) + 0.5 mean angle to the
    other members / 180 (a lone member: 1.0 for the second term)."""
    positions, directions = camera_centres_dirs(views)
    details = {} if details is None else details
    k = analyze_optimal_k(positions, directions, min_cameras, max_cameras, device, details)
    labels, centres, _ = details["fits"][k]        # the reference refits: the same computation, the same result
    _, centre, scale = normalize_positions(positions)
    selected, info, margins = [], {}, []
    for c in range(k):
        idx = np.where(labels == c)[0]
        world = centres[c] * scale + centre
        dist = np.linalg.norm(positions[idx] - world, axis=1)
        if len(idx) > 1:
            ang = _angles_deg(directions[idx])
            # the reference stacks the member in front of the others and takes row 0: the same angles, summed in that order
            uniq = np.array([float(np.mean(np.delete(ang[j], j))) for j in range(len(idx))]) / 180.0
        else:
            uniq = np.ones(len(idx))
        scores = 0.5 * (1.0 / (1.0 + dist)) + 0.5 * uniq
        best = int(np.argmax(scores))
        selected.append(int(idx[best]))
        info[c] = {"members": idx.tolist(), "selected": int(idx[best]), "score": float(scores[best])}
        margins.append(float(scores[best] - np.max(np.delete(scores, best))) if len(idx) > 1 else np.inf)
    details.update(best_k=k, labels=labels, margins=margins)
    return {"selected_indices": selected, "cluster_info": info}


# ---------------------------------------------------------------- process_selected_views.py
def list_images(image_dir):
    """The sorted listing without names that begin with '.' (process_selected_views.py:29-35,131-132)."""
    return [f for f in sorted(os.listdir(image_dir)) if not f.startswith(".")]


def image_path(image_dir, kind, index, files=None):
    """The picture of selected (mapped) index `index`: tyt '%05d.jpg' else '%06d.jpg' (process_selected_views.py:149-164), the
    others entry `index` of list_images.  A missing picture is an error here; the reference warns and shifts the later views."""
    if kind == "tyt":
        for name in (f"{index:05d}.jpg", f"{index:06d}.jpg"):
            if os.path.exists(os.path.join(image_dir, name)):
                return os.path.join(image_dir, name)
        raise FileNotFoundError(f"{image_dir}: neither {index:05d}.jpg nor {index:06d}.jpg exists (view {index})")
    files = list_images(image_dir) if files is None else files
    if not 0 <= index < len(files):
        raise FileNotFoundError(f"{image_dir}: view {index} has no image ({len(files)} images)")
    return os.path.join(image_dir, files[index])


def select_views(camera_path, kind, cluster=True, device=None, details=None):
    """process_views: (selected indices, views).  cluster=False selects every view.  For tyt (whose loader keeps the first half
    of the pose rows) every selected index becomes idx // 2, duplicates included; the mapped index then names the camera AND the
    image, as in the reference."""
    if kind not in KINDS:
        raise ValueError(f"select_views: kind must be one of {KINDS}, got {kind!r}")
    views = load_cameras(camera_path, kind)
    if cluster:
        selected = select_representative_cameras(views, device=device, details=details)["selected_indices"]
    else:
        selected = list(range(len(views)))
    if kind == "tyt":
        selected = [i // 2 for i in selected]
    return [int(i) for i in selected], views
