"""CPU: cilantro_amd/_abi.py, the one place where arrays and tensors cross the C ABI -- its helpers one by one, then every stateless public
wrapper once on a tiny host input: without a device each must still reach the library with a well-formed argument list (ERR_NO_DEVICE)."""
import numpy as np
import pytest
import torch

from cilantro_amd import _abi, capi
from test_stateless_entries_cpu import _has_gpu


# ---- rows ------------------------------------------------------------------------------------------------------------
def test_rows_copies_a_float64_nested_list_to_float32():
    r = _abi.rows([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], 3, "clouds")
    assert isinstance(r.keep, np.ndarray) and r.keep.dtype == np.float32 and r.keep.flags.c_contiguous
    assert (r.n, r.dim, r.mem) == (2, 3, capi.MEM_HOST) and r.ptr == r.keep.ctypes.data
    assert np.array_equal(r.keep, np.array([[1, 2, 3], [4, 5, 6]], np.float32))


def test_rows_keeps_the_copy_of_a_non_contiguous_array():
    a = np.arange(24, dtype=np.float32).reshape(4, 6)[:, ::2]
    r = _abi.rows(a, 3, "clouds")
    assert r.keep is not a and r.keep.flags.c_contiguous and not np.shares_memory(r.keep, a)
    assert r.ptr == r.keep.ctypes.data and np.array_equal(r.keep, a)
    b = np.ascontiguousarray(a)
    assert _abi.rows(b, 3).keep is b      # (and no copy where none is needed)


def test_rows_hands_a_cpu_float32_tensor_over_as_host_memory_without_a_copy():
    t = torch.arange(15, dtype=torch.float32).reshape(5, 3)
    for cast in (False, True):
        r = _abi.rows(t, 3, "clouds", cast=cast)
        assert r.mem == capi.MEM_HOST and r.ptr == t.data_ptr() and (r.n, r.dim) == (5, 3) and isinstance(r.keep, np.ndarray)


def test_rows_float64_tensor_raises_or_converts_by_the_law():
    t = torch.arange(15, dtype=torch.float64).reshape(5, 3)
    with pytest.raises(TypeError, match="^clouds must be float32$"):
        _abi.rows(t, 3, "clouds")
    with pytest.raises(TypeError, match="^points must be float32$"):
        _abi.rows(t, 3)
    r = _abi.rows(t, None, "the points", cast=True)
    assert r.keep.dtype == np.float32 and r.mem == capi.MEM_HOST and r.ptr != t.data_ptr() and np.array_equal(r.keep, t.numpy().astype(np.float32))
    a = _abi.rows(np.arange(6, dtype=np.float64).reshape(2, 3), 3)      # (an array is converted under either law)
    assert a.keep.dtype == np.float32


@pytest.mark.parametrize("make", (np.asarray, torch.as_tensor), ids=("numpy", "torch"))
def test_rows_wrong_rank_or_width_raises_the_texts_users_see(make):
    flat, wide = make(np.zeros(6, np.float32)), make(np.zeros((2, 4), np.float32))
    for x in (flat, wide):
        with pytest.raises(ValueError, match=r"^clouds must have shape \(N, 3\)$"):
            _abi.rows(x, 3, "clouds")
        with pytest.raises(ValueError, match=r"^points must have shape \(N, 5\)$"):
            _abi.rows(x, 5)
        with pytest.raises(ValueError, match="^points are an n x dim array$"):
            _abi.rows(x, 3, "points", cast=True)
    with pytest.raises(ValueError, match="^the seeds are an n x dim array$"):
        _abi.rows(flat, None, "the seeds", cast=True)
    assert _abi.rows(wide, None, "the seeds", cast=True).dim == 4      # (no width asked for: any width)


def test_rows_of_nothing():
    for x in (np.zeros((0, 3), np.float32), torch.zeros((0, 3))):
        r = _abi.rows(x, 3, "clouds")
        assert (r.n, r.dim, r.mem) == (0, 3, capi.MEM_HOST)
    assert _abi.rows(None, 3, "clouds", none_ok=True) == (None, 0, 0, capi.MEM_HOST, None)
    assert _abi.cloud(None) == (None, 0, capi.MEM_HOST, None)
    with pytest.raises(ValueError, match=r"^points must have shape \(N, 3\)$"):      # (None only where the caller says so)
        _abi.rows(None, 3)


def test_cloud_is_the_tuple_the_icp_module_exports():
    from cilantro_amd import icp

    a = np.zeros((4, 3), np.float32)
    assert icp._as_cloud(a) == (a.ctypes.data, 4, capi.MEM_HOST, a) and icp._as_cloud is _abi.cloud
    T = np.arange(16, dtype=np.float32).reshape(4, 4)
    assert np.array_equal(icp._T_to_abi(T), T.T.reshape(16)) and np.array_equal(icp._T_from_abi(icp._T_to_abi(T)), T)
    assert icp._is_torch(torch.zeros(1)) and not icp._is_torch(a)


# ---- enter, empty, ptr, widen, cut, check, colmajor --------------------------------------------------------------------
def test_enter_leaves_a_host_input_alone():
    assert _abi.enter(np.zeros((2, 3), np.float32), 3) == (3, None)
    assert _abi.enter(None, np.int64(1)) == (1, None)
    assert not _abi.on_device(torch.zeros(1)) and not _abi.on_device(np.zeros(1)) and not _abi.on_device(None)


@pytest.mark.parametrize("dtype", (np.float32, np.float64, np.uint8, np.uint16, np.uint32, np.uint64))
def test_empty_on_the_host_is_numpy_of_that_dtype(dtype):
    for shape in (5, (5,), (4, 3), (0, 3)):
        a = _abi.empty(shape, dtype)
        assert isinstance(a, np.ndarray) and a.dtype == np.dtype(dtype) and a.shape == (np.empty(shape).shape) and a.flags.c_contiguous
    z = _abi.empty((3, 2), dtype, zero=True)
    assert z.dtype == np.dtype(dtype) and not z.any()


def test_empty_names_the_signed_tensor_type_of_each_unsigned_word():
    """the mapping itself needs no device: a CPU torch device shows it"""
    for dtype, want in ((np.uint16, torch.int16), (np.uint32, torch.int32), (np.uint64, torch.int64), (np.float32, torch.float32), (np.float64, torch.float64),
                        (np.uint8, torch.uint8)):
        t = _abi.empty((2, 3), dtype, "cpu")
        assert torch.is_tensor(t) and t.dtype == want and tuple(t.shape) == (2, 3)


def test_ptr():
    a, t = np.zeros(3, np.float32), torch.zeros(3)
    assert _abi.ptr(None) is None and _abi.ptr(a) == a.ctypes.data and _abi.ptr(t) == t.data_ptr()


def test_widen_drops_the_sign():
    a = _abi.widen(np.array([0, 7, 0xFFFFFFFF], np.uint32))
    assert a.dtype == np.int64 and a.tolist() == [0, 7, 4294967295]
    t = _abi.widen(torch.tensor([0, 7, -1], dtype=torch.int32))
    assert t.dtype == torch.int64 and t.tolist() == [0, 7, 4294967295]


@pytest.mark.parametrize("make", (np.asarray, torch.as_tensor), ids=("numpy", "torch"))
def test_cut_copies_less_than_half_and_views_the_rest(make):
    base = np.arange(30, dtype=np.float32).reshape(10, 3)
    buf = make(base.copy())
    shares = (lambda a, b: a.data_ptr() == b.data_ptr()) if torch.is_tensor(buf) else np.shares_memory
    small, large = _abi.cut(buf, 2, 10), _abi.cut(buf, 6, 10)
    assert tuple(small.shape) == (2, 3) and not shares(small, buf) and np.array_equal(np.asarray(small), base[:2])
    assert tuple(large.shape) == (6, 3) and shares(large, buf) and np.array_equal(np.asarray(large), base[:6])
    assert shares(_abi.cut(buf, 5, 10), buf)      # (exactly half: a view)
    assert _abi.cut(None, 2, 10) is None


def test_check_is_silent_on_ok_and_raises_the_code_with_the_entry_prefixed():
    L = capi.load()
    assert _abi.check(capi.OK, "cilhip_anything") is None and _abi.check(capi.OK, None, L) is None
    assert L.cilhip_knn_nd(0, None, 8, None, 8, 3, capi.MEM_HOST, 1, 1.0, None, None, None) == capi.ERR_INVALID      # (leaves a text behind)
    text = L.cilhip_last_error(None).decode()
    assert text and text != "null context"
    with pytest.raises(capi.CilhipError) as e:
        _abi.check(capi.ERR_INVALID, "cilhip_knn_nd", L)
    assert e.value.code == capi.ERR_INVALID and str(e.value) == f"cilhip error {capi.ERR_INVALID}: cilhip_knn_nd: {text}"
    with pytest.raises(capi.CilhipError) as e:
        _abi.check(capi.ERR_UNSUPPORTED, None)
    assert e.value.code == capi.ERR_UNSUPPORTED and str(e.value) == f"cilhip error {capi.ERR_UNSUPPORTED}: {text}"


def test_colmajor_is_the_transpose_in_one_row():
    K = np.arange(9, dtype=np.float64).reshape(3, 3)
    k = _abi.colmajor(K, 3)
    assert k.dtype == np.float32 and k.flags.c_contiguous and np.array_equal(k, K.T.reshape(9))
    assert np.array_equal(_abi.colmajor(list(range(16)), 4), np.arange(16).reshape(4, 4).T.reshape(16))
    assert _abi.colmajor(None, 4) is None


# ---- every stateless public wrapper, once ------------------------------------------------------------------------------
N = 8
_rng = np.random.default_rng(5)
P3 = _rng.random((N, 3), dtype=np.float32)
P5 = _rng.random((N, 5), dtype=np.float32)
NRM = np.tile(np.float32([0, 0, 1]), (N, 1))
KMAT = np.float32([[500, 0, 4], [0, 500, 2], [0, 0, 1]])
DEPTH = np.full((4, 8), 1000, np.uint16)
KNN = (np.tile(np.arange(2, dtype=np.int64), (N, 1)), np.zeros((N, 2), np.float32))
CSR = (np.arange(N + 1, dtype=np.uint64), np.arange(N, dtype=np.uint32), np.ones(N, np.float32))
D2 = ((P3[:, None, :] - P3[None, :, :]) ** 2).sum(-1).astype(np.float32)
EYE4 = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))


def _cl():
    from cilantro_amd import clustering

    return clustering


def _mod(name):
    import importlib

    return importlib.import_module("cilantro_amd." + name)


def _cube3():
    return _mod("spatial").ConvexPolytope3f.from_halfspaces(np.float32([[1, 0, 0, -1], [-1, 0, 0, 0], [0, 1, 0, -1], [0, -1, 0, 0], [0, 0, 1, -1], [0, 0, -1, 0]]).T)


def _fuse():
    model = [np.zeros((2 * N, 3), np.float32) for _ in range(3)] + [np.zeros(2 * N, np.float32)]
    return _mod("fusion").fuse_frame(model, 0, (P3 + np.float32([0, 0, 1]), NRM, P3), np.eye(4, dtype=np.float32), KMAT, 8, 4)


WRAPPERS = {
    "clustering.KMeans3f.cluster": lambda: _cl().KMeans3f(P3).cluster(2, seed=1),
    "clustering.kmeans_assign": lambda: _cl().kmeans_assign(P3, P3[:2]),
    "clustering.KMeansXf.cluster": lambda: _cl().KMeansXf(P5).cluster(2, seed=1),
    "clustering.connected_components": lambda: _cl().connected_components(P3, 0.1, _cl().NormalsProximityEvaluator(NRM, 0.1)),
    "clustering.connected_components_nd": lambda: _cl().connected_components_nd(P5, 0.1, _cl().ColorsProximityEvaluator(P3, 0.5)),
    "clustering.connected_components_from_lists": lambda: _cl().connected_components_from_lists(N, np.arange(N + 1) * 2, KNN[0]),
    "clustering.ConnectedComponentExtraction3f.segment": lambda: _cl().ConnectedComponentExtraction3f(P3).segment(_cl().RadiusNeighborhoodSpecification(0.1)),
    "clustering.ConnectedComponentExtractionXf.segment": lambda: _cl().ConnectedComponentExtractionXf(P5).segment(_cl().RadiusNeighborhoodSpecification(0.1), [0, 1], None, 1, N),
    "clustering.mean_shift": lambda: _cl().mean_shift(P3, 0.5, 10, 0.1, seeds=P3[:3]),
    "clustering.mean_shift_nd": lambda: _cl().mean_shift_nd(P5, 0.5, 10, 0.1, seeds=P5[:3]),
    "clustering.MeanShift3f.cluster": lambda: _cl().MeanShift3f(P3).cluster(0.5, 10, 0.1),
    "clustering.MeanShiftXf.cluster": lambda: _cl().MeanShiftXf(P5).cluster(P5[:3], 0.5, 10, 0.1),
    "clustering.SparseMatrix.from_csr": lambda: _cl().SparseMatrix.from_csr(N, *CSR),
    "clustering.SparseMatrix.from_dense": lambda: _cl().SparseMatrix.from_dense(np.eye(N, dtype=np.float32)),
    "clustering.nn_graph_sparse_matrix": lambda: _cl().nn_graph_sparse_matrix(KNN),
    "clustering.SpectralClustering": lambda: _cl().SpectralClustering(CSR, 2),
    "kd_tree.KDTreeXf.kNNSearch": lambda: _mod("kd_tree").KDTreeXf(P5).kNNSearch(None, 2),
    "kd_tree.KDTree2f.kNNInRadiusSearch": lambda: _mod("kd_tree").KDTree2f(P5[:, :2]).kNNInRadiusSearch(P5[:3, :2], 2, 0.5),
    "kd_tree.KDTreeXf.radiusSearch": lambda: _mod("kd_tree").KDTreeXf(P5).radiusSearch(P5[:3], 0.5),
    "grid_downsampler.grid_downsample": lambda: _mod("grid_downsampler").grid_downsample(P3, 0.25, normals=NRM, colors=P3),
    "grid_downsampler.PointsGridDownsampler3f": lambda: _mod("grid_downsampler").PointsGridDownsampler3f(P3, 0.25),
    "image_conversions.depth_image_to_points": lambda: _mod("image_conversions").RGBDImagesToPointsNormalsColors(np.zeros((4, 8, 3), np.uint8), DEPTH, None, KMAT),
    "image_conversions.points_to_depth_image": lambda: _mod("image_conversions").pointsColorsToRGBDImages(P3, P3, KMAT, None, 8, 4, np.eye(4)),
    "image_conversions.points_to_index_map": lambda: _mod("image_conversions").pointsToIndexMap(P3, KMAT, 8, 4),
    "fusion.fuse_frame": _fuse,
    "principal_component_analysis.PrincipalComponentAnalysis": lambda: _mod("principal_component_analysis").PrincipalComponentAnalysis(P5, subset=[0, 2, 4]),
    "multidimensional_scaling.mds_embedding": lambda: _mod("multidimensional_scaling").MultidimensionalScaling2f(D2),
    "multidimensional_scaling.mds_apply": lambda: _mod("multidimensional_scaling").mds_apply(D2, np.ones((N, 2))),
    "normal_estimation.KDTree3f.kNNSearch": lambda: _mod("normal_estimation").KDTree3f(P3).kNNSearch(None, 2),
    "normal_estimation.KDTree3f.radiusSearch": lambda: _mod("normal_estimation").KDTree3f(P3).radiusSearch(P3[:3], 0.5),
    "normal_estimation.NormalEstimation3f.getNormalsKNN": lambda: _mod("normal_estimation").NormalEstimation3f(P3).getNormalsAndCurvatureKNN(4),
    "normal_estimation.NormalEstimation3f.getNormalsRadius": lambda: _mod("normal_estimation").NormalEstimation3f(P3).getNormalsRadius(0.5),
    "normal_estimation.RobustNormalEstimation3f.getNormalsKNN": lambda: _mod("normal_estimation").RobustNormalEstimation3f(P3).getNormalsAndCurvatureKNN(6),
    "model_estimation.PlaneRANSACEstimator3f.estimate": lambda: _mod("model_estimation").PlaneRANSACEstimator3f(P3).estimate(),
    "model_estimation.PlaneRANSACEstimator3f.estimateModel": lambda: _mod("model_estimation").PlaneRANSACEstimator3f(P3).estimateModel(),
    "model_estimation.PlaneRANSACEstimator3f.countInliers": lambda: _mod("model_estimation").PlaneRANSACEstimator3f(P3).countInliers([[0, 0, 1, 0]]),
    "model_estimation.RigidTransformRANSACEstimator3f.estimate": lambda: _mod("model_estimation").RigidTransformRANSACEstimator3f(P3, P3).estimate(),
    "spatial.ConvexHull3f": lambda: _mod("spatial").ConvexHull3f(P3, True, True),
    "spatial.ConvexHull2f": lambda: _mod("spatial").ConvexHull2f(P5[:, :2]),
    "spatial.getPointSignedDistancesFromFacets": lambda: _cube3().getPointSignedDistancesFromFacets(P3),
    "spatial.getInteriorPointsIndexMask": lambda: _cube3().getInteriorPointsIndexMask(P3),
    "spatial.getInteriorPointIndices": lambda: _mod("spatial").SpaceRegion3f([_cube3()]).getInteriorPointIndices(P3),
    "spatial.FlatConvexHull3f": lambda: _mod("spatial").FlatConvexHull3f(P3),
    "icp.transformPoints": lambda: _mod("icp").transformPoints(EYE4, P3),
    "icp.WarpField": lambda: _mod("icp").WarpField(N, N, KNN, _cl().UnityWeightEvaluator(), KNN, _cl().UnityWeightEvaluator()),
}


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_wrapper_reaches_the_library_with_a_well_formed_call(name):
    if _has_gpu():
        pytest.skip("a GPU is present")
    with pytest.raises(capi.CilhipError) as e:
        WRAPPERS[name]()
    assert e.value.code == capi.ERR_NO_DEVICE, str(e.value)


def test_row_count_mismatches_keep_their_texts():
    cl, short = _cl(), P3[: N - 1]
    rows_text = "^points, normals and colors must have the same number of rows$"
    with pytest.raises(ValueError, match=rows_text):
        _mod("grid_downsampler").grid_downsample(P3, 0.25, normals=short)
    with pytest.raises(ValueError, match=rows_text):
        _mod("grid_downsampler").PointsColorsGridDownsampler3f(P3, short, 0.25)
    with pytest.raises(ValueError, match=rows_text):
        cl.connected_components(P3, 0.1, cl.NormalsProximityEvaluator(short, 0.1))
    nd_text = "^the normals are an n x dim array and the colours an n x 3 array over the points' n$"
    with pytest.raises(ValueError, match=nd_text):
        cl.connected_components_nd(P5, 0.1, cl.ColorsProximityEvaluator(short, 0.5))
    with pytest.raises(ValueError, match=nd_text):
        cl.connected_components_nd(P5, 0.1, cl.NormalsProximityEvaluator(P3, 0.1))      # (normals of another width)
    with pytest.raises(ValueError, match="^points and seeds must have the same dimension$"):
        cl.mean_shift_nd(P5, 0.5, 10, 0.1, seeds=P3)
    with pytest.raises(ValueError, match=r"^clouds must have shape \(N, 3\)$"):
        cl.mean_shift(P3, 0.5, 10, 0.1, seeds=P5)
    with pytest.raises(ValueError, match="^offsets must have n \\+ 1 entries and keep one byte per list entry$"):
        cl.connected_components_from_lists(N, np.arange(N) * 2, KNN[0])
    with pytest.raises(ValueError, match="^points and colors must have the same number of rows and live in the same memory space$"):
        _mod("image_conversions").pointsColorsToRGBDImages(P3, short, KMAT, None, 8, 4)


def test_public_names_keep_their_import_paths():
    from cilantro_amd import clustering, kd_tree

    assert clustering.RadiusNeighborhoodSpecification is kd_tree.RadiusNeighborhoodSpecification
    assert clustering.RadiusNeighborhoodSpecification(0.25).radius == 0.25
