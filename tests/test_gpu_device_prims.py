"""GPU: the edges the shared helpers of csrc/device_prims.hpp own, through the entries that use them.  Everything is an integer
result compared with np.array_equal.
  grouping            group_by_label / key_bits / k_iota / k_run_offsets: labels -> offsets[] + members[] with exactly 1, 2, 255, 256 and
                      257 groups (the sort's end bit goes from 1 to 2 and from 8 to 9 bits there), through the components lists entry
                      (reference: tests/_cc_refs.py) and mean shift's grouping (reference: tests/_meanshift_refs.py)
  ordered compaction  block_rank / k_scan_counts: the inlier index lists of plane and transform RANSAC around one wave, one block and
                      one chunk, against np.flatnonzero of a mask that does not hang on rounding"""
import numpy as np
import pytest

import _cc_refs as CR
import _meanshift_refs as MR

pytestmark = pytest.mark.gpu

LABEL_COUNTS = (1, 2, 255, 256, 257)
POINT_COUNTS = (1, 63, 64, 65, 256, 257)
# (points, groups): every point count that can hold the group count, and one more per 8 | 9-bit count with room for ungrouped points
GROUP_CASES = [(n, k) for k in LABEL_COUNTS for n in POINT_COUNTS if n >= k] + [(2 * k + 3, k) for k in (255, 256, 257)]
# one case in device memory per family: the 9-bit label with ungrouped points behind it
DEVICE_CASE = (515, 256)


@pytest.fixture(scope="module")
def cl():
    from cilantro_amd import clustering

    return clustering


def _ids(c):
    return f"n{c[0]}-k{c[1]}"


# ---- components: lists entry ---------------------------------------------------------------------------------------------------------
def _chains(n, k):
    """symmetric CSR lists over n points: the first m form k chains i ~ i + k (point i is in chain i % k), the last n - m are alone.
    -> (offsets, idx, min_segment_size, ungrouped): with room for it (n > 2 k) every chain has two members or more, up to three points
    stay alone and min_segment_size = 2 leaves them without a segment: their label is k, the largest key of the members' sort."""
    alone = min(3, n - 2 * k) if n > 2 * k else 0
    m = n - alone
    lists = [[j for j in (i - k, i + k) if 0 <= j < m] if i < m else [] for i in range(n)]
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    idx = np.array([j for x in lists for j in x], np.uint32)
    return offsets, idx, (2 if alone else 1), alone


def _components(cl, n, k, device_mem):
    offsets, idx, min_size, alone = _chains(n, k)
    want = CR.components_from_lists(n, offsets, idx, skip_first=False, min_segment_size=min_size)
    assert len(want[1]) - 1 == k and int((want[0] == k).sum()) == alone      # the fixture has the group count it is named for
    if device_mem:
        import torch

        # (an empty index array has no device pointer worth passing: every device case has entries)
        got = cl.connected_components_from_lists(n, torch.from_numpy(offsets).cuda(), torch.from_numpy(idx).cuda(), skip_first=False, min_segment_size=min_size)
        assert all(g.is_cuda for g in got)
        got = [g.cpu().numpy() for g in got]
    else:
        got = cl.connected_components_from_lists(n, offsets, idx, skip_first=False, min_segment_size=min_size)
    labels, offs, members = got
    for name, g, w in zip(("labels", "offsets", "members"), got, want):
        assert np.array_equal(g, w), (name, n, k)
    assert len(offs) == k + 1 and offs[k] == n - alone      # the members of the k segments; the ungrouped points follow them
    assert members.shape[0] == n and np.array_equal(np.sort(members), np.arange(n))


@pytest.mark.parametrize("case", GROUP_CASES, ids=_ids)
def test_components_offsets_and_members_at_the_label_bit_boundaries(cl, case):
    _components(cl, *case, device_mem=False)


def test_components_offsets_and_members_in_device_memory(cl):
    _components(cl, *DEVICE_CASE, device_mem=True)


# ---- mean shift: grouping alone (max_iter = 0) ---------------------------------------------------------------------------------------
def _clustered_seeds(n, k):
    """n seeds in k well-separated clusters on a lattice: seed i belongs to cluster i % k, whose first member (seed i % k, the leader)
    sits on the unit lattice; the others are 2^-12 apart behind it, at most 2^-4 away, against a tolerance of 2^-3.  Every squared
    distance inside a cluster is exact in f32 and at most 2^-8 (tolerance^2 = 2^-6); between clusters it is at least 0.75."""
    i = np.arange(n)
    c = i % k
    s = np.zeros((n, 3), np.float32)
    s[:, 0] = c % 16
    s[:, 2] = c // 16
    s[:, 1] = (i // k) * 2.0 ** -12
    return s, np.float32(2.0 ** -3)


def _mean_shift_grouping(cl, n, k, device_mem):
    from test_gpu_mean_shift import run

    seeds, tol = _clustered_seeds(n, k)
    labels, leaders = MR.first_fit(seeds, tol)
    assert len(leaders) == k
    offsets, members = MR.lists_of(labels, k)
    got = run(cl, np.zeros((3, 3), np.float32), seeds, 1.0, 0, tol, device_mem=device_mem)
    assert got["iterations"] == 0
    for name, w in (("labels", labels), ("offsets", offsets), ("members", members)):
        assert np.array_equal(got[name], w), (name, n, k)
    assert len(got["offsets"]) == k + 1 and got["offsets"][k] == n
    assert np.array_equal(got["members"][got["offsets"][:-1]], leaders)


@pytest.mark.parametrize("case", [c for c in GROUP_CASES if c[0] <= 257], ids=_ids)
def test_mean_shift_offsets_and_members_at_the_label_bit_boundaries(cl, case):
    _mean_shift_grouping(cl, *case, device_mem=False)


def test_mean_shift_offsets_and_members_in_device_memory(cl):
    _mean_shift_grouping(cl, 257, 256, device_mem=True)


# ---- RANSAC: the ordered inlier index lists -----------------------------------------------------------------------------------------
COMPACTION_NS = (63, 64, 65, 255, 256, 257, 1025)


def _mask_and_xy(n):
    """every third point is an outlier; x, y on the 2^-10 lattice.  The points 0, 1 and 3 are inliers and not collinear."""
    rng = np.random.default_rng(n)
    xy = (rng.integers(0, 1024, (n, 2)) * 2.0 ** -10).astype(np.float32)
    xy[:4] = [[0.0, 0.0], [1.0, 0.0], [0.5, 0.5], [0.0, 1.0]]
    return np.arange(n) % 3 != 2, xy


SAMPLE = np.array([[0, 1, 3]], np.uint32)


@pytest.mark.parametrize("n", COMPACTION_NS)
def test_plane_ransac_inlier_list_is_the_ascending_mask(hip_lib, n):
    """inliers on the plane z = 0 (residual 0 for the plane through three of them), outliers at distance 1, threshold 0.1"""
    from cilantro_amd.model_estimation import PlaneRANSACEstimator3f

    mask, xy = _mask_and_xy(n)
    x = np.ascontiguousarray(np.column_stack([xy, np.where(mask, 0.0, 1.0)]).astype(np.float32))
    pe = (PlaneRANSACEstimator3f(x).setMaxInlierResidual(0.1).setTargetInlierCount(n).setMaxNumberOfIterations(1).setReEstimationStep(False)
          .setSamples(SAMPLE).estimate())
    want = np.flatnonzero(mask)
    got = pe.getModelInliers()
    print(f"n={n}: {len(got)} inliers listed, {len(want)} expected; largest inlier residual {pe.getModelResiduals()[mask].max():.3e}")
    assert np.array_equal(got, want)
    assert pe.getNumberOfInliers() == len(want)


@pytest.mark.parametrize("n", COMPACTION_NS)
def test_transform_ransac_inlier_list_is_the_ascending_mask(hip_lib, n):
    """inliers with dst == src (the identity fits them), outliers moved by 1 along x, threshold 0.1"""
    from cilantro_amd.model_estimation import RigidTransformRANSACEstimator3f

    mask, xy = _mask_and_xy(n)
    src = np.ascontiguousarray(np.column_stack([xy, (np.arange(n) % 7) * 2.0 ** -3]).astype(np.float32))
    dst = src.copy()
    dst[~mask, 0] += np.float32(1.0)
    te = (RigidTransformRANSACEstimator3f(dst, src).setMaxInlierResidual(0.1).setTargetInlierCount(n).setMaxNumberOfIterations(1)
          .setReEstimationStep(False).setSamples(SAMPLE).estimate())
    want = np.flatnonzero(mask)
    got = te.getModelInliers()
    print(f"n={n}: {len(got)} inliers listed, {len(want)} expected; largest inlier residual {te.getModelResiduals()[mask].max():.3e}")
    assert np.array_equal(got, want)
    assert te.getNumberOfInliers() == len(want)
