"""GPU: what every stateless wrapper hands back, for numpy input and for the same data as device tensors -- through the public API only.

Per wrapper one row: the kind (numpy array or tensor on cuda:0), dtype and shape of every returned object against the literal table SIG below
(written from the wrappers' code as it stood before the marshalling moved into cilantro_amd/_abi.py), and the values of the two calls against
each other, bit for bit: both paths run the same kernels on the same bytes.  300 points: more than one 256-thread block; dim 3, and dim 5 for
the wrappers that take any dimension."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D = 300, 5
H, W = 15, 20            # H * W == N: one pixel per point
F32, I64, U32, U64, U8, F64 = "float32", "int64", "uint32", "uint64", "uint8", "float64"
HOST = None              # "the result is numpy on both paths"


def _blobs(dim, seed):
    rng = np.random.default_rng(seed)
    centres = np.zeros((3, dim), np.float32)
    centres[1, 0] = centres[2, 1] = 2.0
    return (np.repeat(centres, N // 3, axis=0) + rng.normal(0.0, 0.15, (N, dim))).astype(np.float32)


P3, P5 = _blobs(3, 7), _blobs(D, 8)
NRM = np.tile(np.float32([0, 0, 1]), (N, 1))
NRM[::3] = np.float32([0, 1, 0])
RGB = np.random.default_rng(9).random((N, 3), dtype=np.float32)
KMAT = np.float32([[20, 0, 10], [0, 20, 7.5], [0, 0, 1]])
DEPTH = (1000 + 40 * np.add.outer(np.arange(H), np.arange(W))).astype(np.uint16)
DEPTH[2, 3] = 0          # an invalid pixel: the result is shorter than the image
IMAGE = np.random.default_rng(10).integers(0, 256, (H, W, 3), dtype=np.uint8)
CAMERA_PTS = np.stack([np.tile(np.linspace(-0.4, 0.4, W), H), np.repeat(np.linspace(-0.3, 0.3, H), W), np.linspace(1.0, 2.0, N)], axis=1).astype(np.float32)


def host(a):
    return a


def dev(a):
    """the same bytes as a tensor on cuda:0 (unsigned words travel in the signed type of their width)"""
    import torch

    if a is None:
        return None
    a = np.ascontiguousarray(a)
    signed = {"uint16": np.int16, "uint32": np.int32, "uint64": np.int64}.get(a.dtype.name)
    return torch.from_numpy(a.view(signed) if signed else a).cuda()


def _cl():
    from cilantro_amd import clustering

    return clustering


def _tree3():
    from cilantro_amd.normal_estimation import KDTree3f

    return KDTree3f(P3)


# ---- the rows: (put, on_device) -> {name: returned object} ------------------------------------------------------------------------
def kmeans3f(put, on_device):
    km = _cl().KMeans3f(put(P3)).cluster(P3[::100], 20)
    return {"centroids": km.getClusterCentroids(), "labels": km.getPointToClusterIndexMap(), "iterations": km.getNumberOfPerformedIterations(),
            "assign": _cl().kmeans_assign(put(P3), P3[::100])}


def kmeans_xf(put, on_device):
    km = _cl().KMeansXf(put(P5)).cluster(P5[::100], 20)
    return {"centroids": km.getClusterCentroids(), "labels": km.getPointToClusterIndexMap(), "iterations": km.getNumberOfPerformedIterations()}


def _segments(r):
    return dict(zip(("labels", "offsets", "members"), r))


def components3f(put, on_device):
    cl = _cl()
    return _segments(cl.connected_components(put(P3), 0.2 ** 2, cl.PointsNormalsColorsProximityEvaluator(put(NRM), put(RGB), 0.2, 0.1, 2.0), 2, N, seeds=[0, 150, 299]))


def components_nd(put, on_device):
    cl = _cl()
    return _segments(cl.connected_components_nd(put(P5), 0.3 ** 2, cl.NormalsColorsProximityEvaluator(put(P5), put(RGB), 3.0, 2.0), 2))


def components_lists(put, on_device):
    off, idx, _ = _tree3().radiusSearch(None, 0.1 ** 2)
    keep = (np.arange(len(idx)) % 7 != 0).astype(np.uint8)
    return _segments(_cl().connected_components_from_lists(N, put(off), put(idx), put(keep), symmetric=False))


def _extraction(cce):
    return {"labels": cce.getPointToClusterIndexMap(), "clusters": cce.getNumberOfClusters(), "first": cce.getClusterToPointIndicesMap()[0],
            "labeled": cce.getLabeledPointIndices(), "unlabeled": cce.getUnlabeledPointIndices()}


def extraction3f(put, on_device):
    cl = _cl()
    return _extraction(cl.ConnectedComponentExtraction3f(put(P3)).segment(cl.RadiusNeighborhoodSpecification(0.1 ** 2), cl.NormalsProximityEvaluator(put(NRM), 0.1), 3, N))


def extraction_xf(put, on_device):
    cl = _cl()
    cce = cl.ConnectedComponentExtractionXf(put(P5), D).segment(cl.RadiusNeighborhoodSpecification(0.3 ** 2), [5, 120, 250], cl.ColorsProximityEvaluator(put(RGB), 2.0), 3, N)
    assert cce.getLastStats()
    return _extraction(cce)


def _shift(r):
    return {k: r[k] for k in ("shifted", "labels", "modes", "offsets", "members", "iterations")}


def mean_shift3f(put, on_device):
    return _shift(_cl().mean_shift(put(P3), 0.6, 50, 0.2, evaluator=_cl().RBFKernelWeightEvaluator(0.5)))


def mean_shift3f_seeds(put, on_device):
    return _shift(_cl().mean_shift(put(P3), 0.6, 50, 0.2, seeds=put(P3[::7])))


def mean_shift_nd(put, on_device):
    return _shift(_cl().mean_shift_nd(put(P5), 0.8, 50, 0.3, seeds=put(P5[::7])))


def _shift_class(ms):
    return {"shifted": ms.getShiftedSeeds(), "modes": ms.getClusterModes(), "labels": ms.getPointToClusterIndexMap(), "clusters": ms.getNumberOfClusters(),
            "first": ms.getClusterToPointIndicesMap()[0], "iterations": ms.getNumberOfPerformedIterations()}


def mean_shift_class3f(put, on_device):
    return _shift_class(_cl().MeanShift3f(put(P3)).cluster(put(P3[::7]), 0.6, 50, 0.2, 1e-6, _cl().UnityWeightEvaluator()))


def mean_shift_class_xf(put, on_device):
    return _shift_class(_cl().MeanShiftXf(put(P5), D).cluster(0.8, 50, 0.3))


def _knn_lists():
    idx, d2, _ = _tree3().kNNSearch(None, 8)
    return idx, d2


def sparse_from_csr(put, on_device):
    cl = _cl()
    with_graph = cl.nn_graph_sparse_matrix(_knn_lists(), cl.RBFKernelWeightEvaluator(0.3), True)
    off, col, val = with_graph.get()
    M = cl.SparseMatrix.from_csr(N, put(off), put(col), put(val))
    return dict(zip(("offsets", "columns", "values"), M.get(on_device)), info=M.info()[1])


def nn_graph(put, on_device):
    idx, d2 = _knn_lists()
    M = _cl().nn_graph_sparse_matrix((put(idx), put(d2)), _cl().RBFKernelWeightEvaluator(0.3), True)
    return dict(zip(("offsets", "columns", "values"), M.get()), info=M.info()[1])


def spectral(put, on_device):
    cl = _cl()
    M = cl.nn_graph_sparse_matrix(_knn_lists(), cl.RBFKernelWeightEvaluator(0.3), True)
    emb, ev, info = cl.spectral_embedding(M, 3, False, on_device=on_device, raise_unconverged=False)
    return {"embedded": emb, "eigenvalues": ev, "clusters": info["num_clusters"]}


def kd_tree_xf(put, on_device):
    from cilantro_amd.kd_tree import KDTreeXf

    tree = KDTreeXf(put(P5))
    idx, d2, cnt = tree.kNNInRadiusSearch(put(P5[::3]), 6, 0.3 ** 2)
    off, ridx, rd2 = tree.radiusSearch(None, 0.3 ** 2)
    nn, nn_d2 = tree.nearestNeighborSearch(put(P5[::3] + np.float32(0.01)))
    return {"idx": idx, "d2": d2, "cnt": cnt, "offsets": off, "radius_idx": ridx, "radius_d2": rd2, "nn": nn, "nn_d2": nn_d2}


def kd_tree3f(put, on_device):
    from cilantro_amd.normal_estimation import KDTree3f

    tree = KDTree3f(put(P3))
    idx, d2, cnt = tree.kNNInRadiusSearch(put(P3[::3]), 6, 0.1 ** 2)
    off, ridx, rd2 = tree.radiusSearch(None, 0.1 ** 2)
    return {"idx": idx, "d2": d2, "cnt": cnt, "offsets": off, "radius_idx": ridx, "radius_d2": rd2}


def normals(put, on_device):
    from cilantro_amd.normal_estimation import NormalEstimation3f

    ne = NormalEstimation3f(put(P3)).setViewPoint([0, 0, 5])
    nrm, cur = ne.getNormalsAndCurvatureKNN(10)
    rn, rc = ne.getNormalsAndCurvatureRadius(0.2)
    return {"normals": nrm, "curvature": cur, "radius_normals": rn, "radius_curvature": rc}


def robust_normals(put, on_device):
    from cilantro_amd.normal_estimation import RobustNormalEstimation3f

    rne = RobustNormalEstimation3f(put(P3)).setViewPoint([0, 0, 5])
    nrm, cur = rne.getNormalsAndCurvatureKNN(12)
    masks, inliers = rne.getSubsetMasksAndInliersKNN(12)
    return {"normals": nrm, "curvature": cur, "masks": masks, "inliers": inliers}


def grid(put, on_device):
    from cilantro_amd.grid_downsampler import PointsNormalsColorsGridDownsampler3f, grid_downsample

    coarse = grid_downsample(put(P3), 1.0, normals=put(NRM), colors=put(RGB))      # few bins: the results are copies
    ds = PointsNormalsColorsGridDownsampler3f(put(P3), put(NRM), put(RGB), 0.05)    # many bins: the results are views
    p, n, c = ds.getDownsampledPointsNormalsColors()
    return {"coarse_points": coarse["points"], "coarse_normals": coarse["normals"], "coarse_colors": coarse["colors"], "points": p, "normals": n, "colors": c,
            "counts": ds.getBinPointCounts(), "bins": ds.getNumberOfOccupiedBins(), "twice": ds.getDownsampledPoints(2)}


def images_to_points(put, on_device):
    from cilantro_amd import image_conversions as ic

    p, n, c = ic.RGBDImagesToPointsNormalsColors(put(IMAGE), put(DEPTH), ic.DepthValueConverter(1000.0), KMAT, np.eye(4))
    full = ic.depthImageToPoints(put(DEPTH.astype(np.float32)), ic.TruncatedDepthValueConverter(1000.0, 1.5), KMAT, keep_invalid=True)
    return {"points": p, "normals": n, "colors": c, "full": full}


def points_to_images(put, on_device):
    from cilantro_amd import image_conversions as ic

    rgb, depth = ic.pointsColorsToRGBDImages(put(CAMERA_PTS), put(RGB), KMAT, ic.DepthValueConverter(1000.0), W, H)
    metric = ic.pointsToDepthImage(put(CAMERA_PTS), KMAT, None, W, H, np.eye(4), np.float32)
    return {"rgb": rgb, "depth": depth, "metric": metric, "index": ic.pointsToIndexMap(put(CAMERA_PTS), KMAT, W, H)}


def fuse(put, on_device):
    from cilantro_amd import fusion

    model = [put(np.zeros((2 * N, 3), np.float32)) for _ in range(3)] + [put(np.zeros(2 * N, np.float32))]
    n_out, counts = fusion.fuse_frame(model, 0, (put(CAMERA_PTS), put(NRM), put(RGB)), np.eye(4, dtype=np.float32), KMAT, W, H)
    n_out, again = fusion.fuse_frame(model, n_out, (put(CAMERA_PTS), put(NRM), put(RGB)), np.eye(4, dtype=np.float32), KMAT, W, H)
    return {"rows": n_out, "appended": counts["appended"], "fused": again["fused"], "points": model[0][:n_out], "normals": model[1][:n_out], "colors": model[2][:n_out],
            "confidence": model[3][:n_out]}


def pca(put, on_device):
    from cilantro_amd.principal_component_analysis import PrincipalComponentAnalysis

    fit = PrincipalComponentAnalysis(put(P5), subset=np.arange(0, N, 2))
    low = fit.project(put(P5), 2)
    return {"mean": fit.getDataMean(), "covariance": fit.getDataCovariance(), "eigenvalues": fit.getEigenValues(), "eigenvectors": fit.getEigenVectors(), "low": low,
            "back": fit.reconstruct(low)}


def mds(put, on_device):
    from cilantro_amd import multidimensional_scaling as m

    d2 = ((P3[:, None, :2] - P3[None, :, :2]) ** 2).sum(-1).astype(np.float32)
    emb, ev, info = m.mds_embedding(put(d2), 2, raise_unconverged=False)
    y, _ = m.mds_apply(put(d2), put(np.ones((N, 2))))
    return {"embedded": emb, "eigenvalues": ev, "dim": info["dim"], "product": y}


def ransac(put, on_device):
    from cilantro_amd.model_estimation import PlaneRANSACEstimator3f

    flat = P3 * np.float32([1, 1, 0.02])
    pe = PlaneRANSACEstimator3f(put(flat)).setMaxInlierResidual(0.01).setSeed(3).estimate()
    return {"model": pe.getModel(), "residuals": pe.getModelResiduals(), "inliers": pe.getModelInliers(), "fit": pe.estimateModel(),
            "counts": pe.countInliers([[0, 0, 1, 0], [1, 0, 0, 0]])}


def hull(put, on_device):
    from cilantro_amd.spatial import ConvexHull3f, SpaceRegion3f

    h = ConvexHull3f(put(P3[:100]), True, True)
    region = SpaceRegion3f([h, ConvexHull3f(P3[100:200])])
    return {"vertices": h.getVertices(), "vertex_points": h.getVertexPointIndices(), "hyperplanes": h.getFacetHyperplanes(),
            "distances": h.getPointSignedDistancesFromFacets(put(P3)), "mask": h.getInteriorPointsIndexMask(put(P3), 0.01), "inside": region.getInteriorPointIndices(put(P3))}


ROWS = {f.__name__: f for f in (kmeans3f, kmeans_xf, components3f, components_nd, components_lists, extraction3f, extraction_xf, mean_shift3f, mean_shift3f_seeds,
                                mean_shift_nd, mean_shift_class3f, mean_shift_class_xf, sparse_from_csr, nn_graph, spectral, kd_tree_xf, kd_tree3f, normals, robust_normals,
                                grid, images_to_points, points_to_images, fuse, pca, mds, ransac, hull)}

# ---- the table: name -> (numpy dtype, tensor dtype for device input or HOST, shape; None: whatever the data give, the same on both paths) -----
INT = "a Python int"
MAY_BE_EMPTY = ("unlabeled", "twice")
NS, NQ = len(P3[::7]), len(P3[::3])
_SEGMENTS = {"labels": (I64, I64, (N,)), "offsets": (I64, I64, (None,)), "members": (I64, I64, (N,))}
_EXTRACTION = {"labels": (I64, I64, (N,)), "clusters": INT, "first": (I64, I64, (None,)), "labeled": (I64, I64, (None,)), "unlabeled": (I64, I64, (None,))}


def _shift_sig(ns, dim):
    return {"shifted": (F32, F32, (ns, dim)), "labels": (I64, I64, (ns,)), "modes": (F32, F32, (None, dim)), "offsets": (I64, I64, (None,)), "members": (I64, I64, (ns,)),
            "iterations": INT}


def _shift_class_sig(ns, dim):
    return {"shifted": (F32, F32, (ns, dim)), "modes": (F32, F32, (None, dim)), "labels": (I64, I64, (ns,)), "clusters": INT, "first": (I64, I64, (None,)), "iterations": INT}


_CSR = {"offsets": (U64, "int64", (N + 1,)), "columns": (U32, "int32", (None,)), "values": (F32, F32, (None,)), "info": INT}
SIG = {
    "kmeans3f": {"centroids": (F32, HOST, (3, 3)), "labels": (I64, HOST, (N,)), "iterations": INT, "assign": (I64, HOST, (N,))},
    "kmeans_xf": {"centroids": (F32, HOST, (3, D)), "labels": (I64, HOST, (N,)), "iterations": INT},
    "components3f": _SEGMENTS, "components_nd": _SEGMENTS, "components_lists": _SEGMENTS,
    "extraction3f": _EXTRACTION, "extraction_xf": _EXTRACTION,
    "mean_shift3f": _shift_sig(N, 3), "mean_shift3f_seeds": _shift_sig(NS, 3), "mean_shift_nd": _shift_sig(NS, D),
    "mean_shift_class3f": _shift_class_sig(NS, 3), "mean_shift_class_xf": _shift_class_sig(N, D),
    "sparse_from_csr": _CSR,
    "nn_graph": {"offsets": (U64, HOST, (N + 1,)), "columns": (U32, HOST, (None,)), "values": (F32, HOST, (None,)), "info": INT},
    "spectral": {"embedded": (F32, F32, (N, None)), "eigenvalues": (F32, HOST, (None,)), "clusters": INT},
    "kd_tree_xf": {"idx": (I64, HOST, (NQ, 6)), "d2": (F32, HOST, (NQ, 6)), "cnt": (I64, HOST, (NQ,)), "offsets": (I64, HOST, (N + 1,)), "radius_idx": (I64, HOST, (None,)),
                   "radius_d2": (F32, HOST, (None,)), "nn": (I64, HOST, (NQ,)), "nn_d2": (F32, HOST, (NQ,))},
    "kd_tree3f": {"idx": (I64, HOST, (NQ, 6)), "d2": (F32, HOST, (NQ, 6)), "cnt": (I64, HOST, (NQ,)), "offsets": (I64, HOST, (N + 1,)), "radius_idx": (I64, HOST, (None,)),
                  "radius_d2": (F32, HOST, (None,))},
    "normals": {"normals": (F32, HOST, (N, 3)), "curvature": (F32, HOST, (N,)), "radius_normals": (F32, HOST, (N, 3)), "radius_curvature": (F32, HOST, (N,))},
    "robust_normals": {"normals": (F32, F32, (N, 3)), "curvature": (F32, F32, (N,)), "masks": (U32, "int32", (N,)), "inliers": (U8, U8, (N,))},
    "grid": {"coarse_points": (F32, F32, (None, 3)), "coarse_normals": (F32, F32, (None, 3)), "coarse_colors": (F32, F32, (None, 3)), "points": (F32, F32, (None, 3)),
             "normals": (F32, F32, (None, 3)), "colors": (F32, F32, (None, 3)), "counts": (U32, "int32", (None,)), "bins": INT, "twice": (F32, F32, (None, 3))},
    "images_to_points": {"points": (F32, F32, (None, 3)), "normals": (F32, F32, (None, 3)), "colors": (F32, F32, (None, 3)), "full": (F32, F32, (N, 3))},
    "points_to_images": {"rgb": (U8, U8, (H, W, 3)), "depth": ("uint16", "int16", (H, W)), "metric": (F32, F32, (H, W)), "index": (U32, "int32", (H, W))},
    "fuse": {"rows": INT, "appended": INT, "fused": INT, "points": (F32, F32, (None, 3)), "normals": (F32, F32, (None, 3)), "colors": (F32, F32, (None, 3)),
             "confidence": (F32, F32, (None,))},
    "pca": {"mean": (F32, HOST, (D,)), "covariance": (F32, HOST, (D, D)), "eigenvalues": (F32, HOST, (D,)), "eigenvectors": (F32, HOST, (D, D)), "low": (F32, F32, (N, 2)),
            "back": (F32, F32, (N, D))},
    "mds": {"embedded": (F32, F32, (N, None)), "eigenvalues": (F32, HOST, (None,)), "dim": INT, "product": (F64, F64, (N, 2))},
    "ransac": {"model": (F32, HOST, (4,)), "residuals": (F32, HOST, (N,)), "inliers": (I64, HOST, (None,)), "fit": (F32, HOST, (4,)), "counts": (I64, HOST, (2,))},
    "hull": {"vertices": (F32, HOST, (None, 3)), "vertex_points": (U32, HOST, (None,)), "hyperplanes": (F32, HOST, (4, None)), "distances": (F32, F32, (None, N)),
             "mask": ("bool", "bool", (N,)), "inside": (U32, "int32", (None,))},
}


def test_the_table_names_every_row():
    assert set(SIG) == set(ROWS)


@pytest.mark.parametrize("name", sorted(ROWS))
def test_signature_and_values_for_numpy_and_device_input(name):
    import torch

    got_host, got_dev = ROWS[name](host, False), ROWS[name](dev, True)
    assert set(got_host) == set(got_dev) == set(SIG[name])
    for key, sig in SIG[name].items():
        h, d = got_host[key], got_dev[key]
        if sig == INT:
            assert isinstance(h, int) and isinstance(d, int) and h == d, (key, h, d)
            continue
        np_dtype, tensor_dtype, shape = sig
        assert isinstance(h, np.ndarray) and h.dtype == np.dtype(np_dtype), (key, type(h), getattr(h, "dtype", None))
        assert len(h.shape) == len(shape) and all(want is None or want == have for want, have in zip(shape, h.shape)), (key, h.shape)
        if tensor_dtype is HOST:
            assert isinstance(d, np.ndarray) and d.dtype == h.dtype, (key, type(d), getattr(d, "dtype", None))
        else:
            assert torch.is_tensor(d) and d.is_cuda and d.device.index == 0 and d.dtype == getattr(torch, tensor_dtype), (key, type(d), getattr(d, "dtype", None))
            d = d.cpu().numpy()
        assert tuple(d.shape) == h.shape, (key, d.shape, h.shape)
        assert h.size > 0 or key in MAY_BE_EMPTY, key      # (a row that returns nothing checks nothing)
        assert np.ascontiguousarray(d).tobytes() == np.ascontiguousarray(h).tobytes(), key      # integers equal, floats bit for bit
