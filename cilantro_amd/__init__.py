"""cilantro_amd: Python mirrors of the cilantro classes over libcilantro_hip.so.  Each family lives in its own module; the names below are
also reachable from the package itself (resolved on first use, so importing the package loads nothing)."""

_KD_TREE = ("KDTree", "KDTree2f", "KDTreeXf", "KNNNeighborhoodSpecification", "KNNInRadiusNeighborhoodSpecification")
_MEAN_SHIFT = ("MeanShift3f", "MeanShift2f", "MeanShiftXf", "mean_shift", "mean_shift_nd")
_COMPONENTS_ND = ("ConnectedComponentExtraction2f", "ConnectedComponentExtractionXf", "connected_components_nd")
__all__ = list(_KD_TREE + _MEAN_SHIFT + _COMPONENTS_ND)


def __getattr__(name):
    if name in _KD_TREE:
        from . import kd_tree

        return getattr(kd_tree, name)
    if name in _MEAN_SHIFT or name in _COMPONENTS_ND:
        from . import clustering

        return getattr(clustering, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
