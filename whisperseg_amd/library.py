"""Reading a patches archive back as a LIBRARY: the calls of another folder expressed in the library's call types, on its map and on
its principal axes.  The `.npz` that `scripts/segment.py --patches W --patches_save_path FILE.npz [--clusters ..] [--embed ..]
[--pca ..]` writes holds everything that takes: the pictures (`patch`), their call types and the tree they came from
(`patch_cluster`, `mst_edges`, `mst_weight`: whisperseg_amd.linkage), the map (`embedding`: whisperseg_amd.embed) and the axes
(`pca_mean`, `pca_components`: whisperseg_amd.pca).

`patch_library` reads it; `patch_onto` takes what `segment*(..., patches=W)` returned for the new recordings and gives, per new call,
its nearest library calls and — for whatever the library holds — its call type (linkage.assign_host), its place on the map
(embed.transform) and its scores (pca.project).  Every output of a new call is a function of that call and the library alone: not of
the other calls of the batch, their order or their number.  Nothing of the library moves."""
import numpy as np

from . import embed as EM, linkage as LK, neighbors as NB, pca as PC, resident as RS

KEYS = ("patch", "patch_cluster", "mst_edges", "mst_weight", "embedding", "pca_mean", "pca_components")


def patch_library(archive):
    """{name: numpy array} of what a library is read for (KEYS; those the archive holds) from a patches `.npz` — its path, or an open
    one — or a dict of its arrays.  ValueError unless it holds `patch` float [rows, n_mels, W] and every other array fits its rows."""
    if isinstance(archive, dict):
        found = {key: np.asarray(archive[key]) for key in KEYS if key in archive}
    elif hasattr(archive, "files"):
        found = {key: archive[key] for key in KEYS if key in archive.files}
    else:
        with np.load(archive) as opened:
            found = {key: opened[key] for key in KEYS if key in opened.files}
    if "patch" not in found or found["patch"].ndim != 3:
        raise ValueError('a library holds "patch" [rows, n_mels, W]: the archive of --patches W --patches_save_path FILE.npz')
    found["patch"] = np.ascontiguousarray(found["patch"], dtype=np.float32)
    n = len(found["patch"])
    columns = found["patch"].shape[1] * found["patch"].shape[2]
    if "patch_cluster" in found and found["patch_cluster"].shape != (n,):
        raise ValueError(f'"patch_cluster" must be [rows] = {(n,)} (got {found["patch_cluster"].shape})')
    if "mst_edges" in found or "mst_weight" in found:
        LK.check_tree(found.get("mst_edges", np.zeros((0, 2))), found.get("mst_weight", np.zeros(0)), n)
    if "embedding" in found and (found["embedding"].ndim != 2 or found["embedding"].shape[0] != n or found["embedding"].shape[1] not in (2, 3)):
        raise ValueError(f'"embedding" must be [rows, 2 or 3] (got {found["embedding"].shape})')
    if "pca_components" in found and "pca_mean" in found and len(found["pca_components"]) and (
            found["pca_components"].ndim != 2 or found["pca_components"].shape[1] != columns or found["pca_mean"].shape != (columns,)):
        raise ValueError(f'"pca_mean" must be [{columns}] and "pca_components" [r, {columns}] '
                         f'(got {found["pca_mean"].shape} and {found["pca_components"].shape})')
    return found


def patch_onto(predictions, library, k=15, min_dist=0.1, seed=0, min_samples=5, epochs=EM.PLACE_EPOCHS, device="cuda"):
    """The calls of `predictions` — what segment*(..., patches=W) returned, or the pictures themselves (neighbors.patch_pictures_of):
    the rows of the CLI's CSV — against `library` (patch_library, or what it reads) -> a dict of numpy arrays, one row per new call:
      library_index int32 [rows, k], library_distance float32 [rows, k]   its k nearest library calls (rows of the library; squared
                                   distances, ascending, -1 / +inf where the library has fewer): always there
      patch_cluster int32 [rows]   the library's call type or -1 (linkage.assign_host), if the library has patch_cluster, mst_edges
                                   and mst_weight; `min_samples`: the library's own (lowered to its rows - 1, as it was there)
      embedding float32 [rows, dim]   its place on the library's map (embed.transform), if the library has embedding; `min_dist`,
                                   `seed`: the library's own, `epochs` of placement
      pca_scores float32 [rows, r]   its scores on the library's axes (pca.project), if the library has pca_mean and pca_components
    The library's pictures go to the device once and the lists are computed once, for all three.  ValueError for pictures of another
    shape than the library's, an empty library, or k below min_samples where call types are asked for; every argument is checked
    before anything runs."""
    lib = patch_library(library)
    k = NB.check_k(k)
    EM.curve_ab(min_dist)
    RS.check_int(seed, "seed", 0, EM.MASK, "in 0 .. 2^64 - 1")
    s = RS.check_int(min_samples, "min_samples", 1, LK.MAX_SAMPLES)
    RS.check_int(epochs, "epochs", 1, 2 ** 31 - 1, "of at least 1")
    shape = lib["patch"].shape[1:]
    pictures = NB.patch_pictures_of(predictions, none=shape)
    if tuple(pictures.shape[1:]) != tuple(shape):
        raise ValueError(f"the new pictures are {tuple(pictures.shape[1:])}, the library's {tuple(shape)}: segment with the library's --patches W")
    n, m = len(lib["patch"]), int(pictures.shape[0])
    if n == 0:
        raise ValueError("the library holds no call")
    typed = all(key in lib for key in ("patch_cluster", "mst_edges", "mst_weight"))
    s = min(s, n - 1)
    if typed and k < s:
        raise ValueError(f"k = {k} lists fewer library calls than min_samples = {s} needs")
    mapped = "embedding" in lib
    scored = "pca_mean" in lib and "pca_components" in lib
    if m == 0:
        out = {"library_index": np.zeros((0, k), np.int32), "library_distance": np.zeros((0, k), np.float32)}
        if typed:
            out["patch_cluster"] = np.zeros(0, np.int32)
        if mapped:
            out["embedding"] = np.zeros((0, lib["embedding"].shape[1]), np.float32)
        if scored:
            out["pca_scores"] = np.zeros((0, len(lib["pca_components"])), np.float32)
        return out
    corpus = RS.resident(lib["patch"].reshape(n, -1), device)
    rows = RS.resident(pictures.reshape(m, -1), corpus.device)
    index, distance = (t.cpu().numpy() for t in NB.knn_rows(rows, corpus, k))
    out = {"library_index": index, "library_distance": distance}
    if typed:
        labels = lib["patch_cluster"]
        if s < 1:                                        # a library of one call has no tree and no call type
            out["patch_cluster"] = np.full(m, -1, dtype=np.int32)
        else:
            core = NB.knn_rows(corpus, None, s)[1][:, s - 1].cpu().numpy()
            out["patch_cluster"] = LK.assign_host(index, distance, core, labels, LK.reach_of(lib["mst_edges"], lib["mst_weight"], labels), s)
    if mapped:
        out["embedding"] = EM.transform(rows, corpus, lib["embedding"], k, min_dist, 1.0, epochs, seed, lists=(index, distance), device=device)
    if scored:
        basis = lib["pca_components"]
        out["pca_scores"] = (PC.project_rows(rows, lib["pca_mean"], basis.T).cpu().numpy().astype(np.float32) if len(basis)
                             else np.zeros((m, 0), np.float32))
    return out
