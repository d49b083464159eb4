"""GPU: the common opening of the stateless entry points (csrc/stateless.hpp) -- a cloud the caller already holds on the device gives
the bytes an uploaded one gives, at every entry; a device index the machine does not have is refused with the code each family
always returned, nothing written, and the next call is right; a seeded RANSAC run is the run over the samples the seed draws
(csrc/ransac_sampling.hpp).  The builders and the table of codes are tests/test_stateless_entries_cpu.py's."""
import ctypes as C

import numpy as np
import pytest

from cilantro_amd import capi, synthetic as syn
from test_stateless_entries_cpu import DEVICE, DEVICE_OUT_OF_RANGE, ENTRIES, HOST, INVALID, NO_TEXT, OK, RANSAC, Obj, outputs, pair_clouds, plane_cloud, run

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 257, 20_000)      # below a RANSAC sample (3); one past a block of 256; several blocks


def draw_samples(seed, n, max_iter):
    """csrc/ransac_sampling.hpp restated: min(n, 3) distinct indices per iteration from the splitmix64 stream of `seed`, each draw
    (x * bound) >> 64 among the indices not picked yet; the unused entries of a short sample are 0"""
    size = min(n, 3)
    stream = [int(x) for x in syn.splitmix64(seed, size * max_iter)]
    out = np.zeros((max_iter, 3), np.uint32)
    for it in range(max_iter):
        pick = []
        for i in range(size):
            v = (stream[it * size + i] * (n - i)) >> 64
            for p in sorted(pick):
                v += 1 if v >= p else 0
            pick.append(v)
        out[it, :size] = pick
    return out.reshape(-1)


def build(entry, n, **kw):
    if "kmeans" in entry:
        kw.setdefault("k", min(3, n))
    if entry in RANSAC:
        kw.setdefault("max_iter", 8)
        kw.setdefault("samples", draw_samples(11, n, kw["max_iter"]))
    return ENTRIES[entry](entry, n=n, **kw)


def results(L, entry, args):
    """the outputs of a finished call as bytes (a result struct without its measured time; a shard through its own calls)"""
    out = []
    for a in args:
        if isinstance(a, Obj) and isinstance(a.o, (capi.PlaneModel, capi.TransformModel)):
            a.o.device_ms = 0.0
    if entry == "cilhip_kmeans_shard_create":
        h, m = args[-1].o, C.c_float(-1.0)
        assert L.cilhip_kmeans_shard_maxabs(h, C.byref(m)) == OK
        L.cilhip_kmeans_shard_destroy(h)
        return [bytes(m)]
    out += outputs(args)
    return out


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_device_input_gives_the_bytes_of_host_input(hip_lib, entry):
    L = hip_lib
    for n in SIZES:
        host, dev = build(entry, n, mem=HOST), build(entry, n, mem=DEVICE)
        assert outputs(host) == outputs(dev)      # (the same inputs, the same untouched outputs)
        assert run(L, entry, host) == OK, (n, L.cilhip_last_error(None))
        assert run(L, entry, dev, on_device=True) == OK, (n, L.cilhip_last_error(None))
        assert L.cilhip_last_error(None) == NO_TEXT
        if entry == "cilhip_radius_search3f":
            assert host[-1].o.value <= host[-2], "the lists did not fit: the comparison would see offsets only"
        got_host, got_dev = results(L, entry, host), results(L, entry, dev)
        assert got_host == got_dev, (entry, n)
        if n == SIZES[-1] and entry != "cilhip_kmeans_shard_create":
            assert got_host != outputs(build(entry, n)), "the call wrote nothing"


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_device_index_out_of_range(hip_lib, entry):
    import torch

    L, n = hip_lib, 257
    good = build(entry, n)
    assert run(L, entry, good) == OK, L.cilhip_last_error(None)
    expected = results(L, entry, good)
    for device in (torch.cuda.device_count(), -1):
        args = build(entry, n, device=device)
        before = outputs(args)
        assert run(L, entry, args) == DEVICE_OUT_OF_RANGE[entry], device
        if entry == "cilhip_kmeans_shard_create":
            assert args[-1].o.value is None
        elif entry == "cilhip_radius_search3f":      # (*total_out is reset with the argument rules)
            assert outputs(args)[:-1] == before[:-1] and args[-1].o.value == 0
        else:
            assert outputs(args) == before
        assert b"device" in L.cilhip_last_error(None)
        again = build(entry, n)
        assert run(L, entry, again) == OK, L.cilhip_last_error(None)
        assert results(L, entry, again) == expected
        assert L.cilhip_last_error(None) == NO_TEXT


@pytest.mark.parametrize("entry", RANSAC)
@pytest.mark.parametrize("n", [3, 5000])
def test_seeded_ransac_is_the_run_over_the_samples_its_seed_draws(hip_lib, entry, n):
    L, seed, max_iter = hip_lib, 0x1234567, 40
    P = plane_cloud(n, 5) if entry == "cilhip_plane_ransac3f" else pair_clouds(n, 5)
    samples = draw_samples(seed, n, max_iter)
    tri = samples.reshape(-1, 3)
    assert (tri < n).all() and (tri[:, 0] != tri[:, 1]).all() and (tri[:, 1] != tri[:, 2]).all() and (tri[:, 0] != tri[:, 2]).all()
    seeded = build(entry, n, P=P, samples=None, seed=seed, max_iter=max_iter, target=n)
    explicit = build(entry, n, P=P, samples=samples, seed=0, max_iter=max_iter, target=n)
    assert seeded[4 if entry == "cilhip_plane_ransac3f" else 5] is None and explicit[4 if entry == "cilhip_plane_ransac3f" else 5] is not None
    assert run(L, entry, seeded) == OK and run(L, entry, explicit) == OK, L.cilhip_last_error(None)
    model = seeded[-3].o
    assert model.iterations == max_iter or model.n_inliers == n
    if n > 3:
        assert 3 <= model.n_inliers < n      # a model was accepted, and the outliers stayed out
    assert results(L, entry, seeded) == results(L, entry, explicit)


@pytest.mark.parametrize("entry", RANSAC)
def test_a_sample_index_out_of_range_is_refused(hip_lib, entry):
    L, n = hip_lib, 257
    samples = draw_samples(3, n, 8)
    samples[3 * 5 + 1] = n
    args = build(entry, n, samples=samples)
    before = outputs(args)
    assert run(L, entry, args) == INVALID
    assert b"sample" in L.cilhip_last_error(None)
    assert outputs(args)[1:] == before[1:]      # (residuals and inliers; the model is filled from the host state whatever the status)
    # an unused entry of a short sample may hold anything
    short = draw_samples(3, 2, 8)
    short[2::3] = 0xFFFFFFFF
    assert run(L, entry, build(entry, 2, samples=short)) == OK, L.cilhip_last_error(None)
