"""CPU: the comparison targets of tests/test_gpu_cloud_frames.py are themselves exact on the clouds that test builds -- a unit cube
moved to 16384 on every axis (coordinates quantised at 2^-9 against a point spacing of 0.02: exact ties) and the same cube rescaled by
2^-24 and 2^24.  The oracle kd-tree and the reference's nanoflann (where oracle/_ref is built) must name the exhaustive argmin
under the pinned d2 of every query, up to exact ties, so a mismatch the GPU test reports can only be the kernel's."""
import numpy as np

from cilantro_amd import synthetic as syn


def _moved(d, scale=1.0, offset=0.0):
    f = lambda a: np.ascontiguousarray((a.astype(np.float64) * scale + offset).astype(np.float32))
    return f(d["dst"]), f(d["src"]), np.float32(float(d["max_sq_dist"]) * scale * scale)


def test_kd_trees_are_exact_on_offset_and_rescaled_clouds(orc):
    base = syn.make_pair(120_000, 12_000)
    report = {}
    for name, scale, offset in (("offset 16384", 1.0, 16384.0), ("scale 2^-24", 2.0 ** -24, 0.0), ("scale 2^24", 2.0 ** 24, 0.0)):
        D, S, r2 = _moved(base, scale, offset)
        bi, bd = orc.nn_brute(D, S, float(r2))
        assert np.count_nonzero(bi >= 0) > 0.9 * len(S), name
        trees = [("oracle kd-tree", orc.KDTree(D))]
        if orc.ref_available():
            trees.append(("reference nanoflann", orc.KDTree(D, use_ref=True)))
        for tname, tree in trees:
            o1, o2, ov = tree.find_correspondences(S, float(r2))
            oi = np.full(len(S), -1, np.int64); od = np.zeros(len(S), np.float32)
            oi[o2] = o1; od[o2] = ov
            assert np.array_equal(oi >= 0, bi >= 0), (name, tname)
            m = bi >= 0
            assert np.array_equal(od[m].view(np.uint32), bd[m].view(np.uint32)), (name, tname)   # the smallest pinned d2, bit for bit
            ties = int(np.count_nonzero(oi != bi))
            # a different index only where the brute-force distance is reached by both points (an exact tie)
            if ties:
                diff = np.nonzero(oi != bi)[0]
                alt = ((D[oi[diff]] - S[diff]) ** 2)
                assert np.array_equal(((alt[:, 0] + alt[:, 1]) + alt[:, 2]).view(np.uint32), bd[diff].view(np.uint32)), (name, tname)
            report[(name, tname)] = ties
        if name == "offset 16384":
            assert orc.count_ties_brute(D, S, float(r2)) > 0        # the regime the ties are meant to exercise
        else:
            assert all(v == 0 for (n, _), v in report.items() if n == name), report
    # rescaling by a power of two changes no index and scales every d2 exactly
    D0, S0, r20 = _moved(base)
    b0, d0 = orc.nn_brute(D0, S0, float(r20))
    for k in (-24, 24):
        D, S, r2 = _moved(base, 2.0 ** k)
        bi, bd = orc.nn_brute(D, S, float(r2))
        assert np.array_equal(bi, b0)
        m = b0 >= 0
        assert np.array_equal(bd[m].view(np.uint32), (d0[m] * np.float32(4.0 ** k)).view(np.uint32)), k
