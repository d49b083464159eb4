"""CPU: the yardstick of the rigid-fit tests (tests/_rigid_refs.py) can fail -- three wrong fits that check() must refuse -- and the
host build of kabsch_from_sums (cilantro_amd/csrc/solve.hpp, through tests/cpp/rigid_fit_host.cpp) passes it on the whole case table
in every frame, which pins the table and the derived bound without a GPU.  The same program reports which branch each case takes:
the polar iteration or the SVD fallback."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _rigid_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build_host_fit():
    """tests/cpp/rigid_fit_host.cpp with hipcc, as tests/cpp/build.sh builds test_solve (the header pulls in the HIP runtime API)"""
    out_dir = os.path.join(HERE, "cpp", "bin")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "rigid_fit_host")
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", os.path.join(HERE, "cpp", "rigid_fit_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def host_fit(exe, sets, tmp_path):
    """[(dst, src)] -> [(T 4x4 f32, took the polar branch)]"""
    path = os.path.join(str(tmp_path), "pairs.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(sets)))
        for d, s in sets:
            f.write(struct.pack("<I", len(d)))
            f.write(np.ascontiguousarray(d, np.float32).tobytes())
            f.write(np.ascontiguousarray(s, np.float32).tobytes())
    r = subprocess.run([exe, path], capture_output=True, timeout=120)
    assert r.returncode == 0 and len(r.stdout) == 68 * len(sets), (r.returncode, len(r.stdout), r.stderr[-500:])
    out = []
    for k in range(len(sets)):
        T = np.frombuffer(r.stdout, np.float32, 16, 68 * k).reshape(4, 4).T.copy()
        out.append((T, bool(np.frombuffer(r.stdout, np.int32, 1, 68 * k + 64)[0])))
    return out


@pytest.fixture(scope="module")
def exe():
    return build_host_fit()


def test_the_optimum_passes_its_own_check():
    for fi, (fname, _, _) in enumerate(R.FRAMES):
        for name, d, s in R.cases(fi):
            _, _, Ro, to = R.optimum(d, s)
            R.check(R.pack(Ro, to), d, s, f"{fname}/{name}")


def test_a_reflection_fails():
    """the optimal orthogonal matrix without the flip: det -1 on every mirrored 500-pair case"""
    for fi, (fname, _, _) in enumerate(R.FRAMES):
        seen = 0
        for name, d, s in R.cases(fi):
            if name in R.MIRRORED_500:
                _, _, Rn, tn = R.optimum(d, s, flip=False)
                assert np.linalg.det(Rn) < 0
                assert not R.passes(R.pack(Rn, tn), d, s), (fname, name)
                seen += 1
        assert seen == len(R.MIRRORED_500)


def test_the_flip_on_the_wrong_column_fails():
    """a proper rotation, but column 0 of U negated instead of column 2: the largest singular value enters with the wrong sign"""
    for fi, (fname, _, _) in enumerate(R.FRAMES):
        name, d, s = [c for c in R.cases(fi) if c[0] == "500 mirrored, 1e-3 noise"][0]
        _, _, Rw, tw = R.optimum(d, s, flip_col=0)
        assert np.linalg.det(Rw) > 0
        assert not R.passes(R.pack(Rw, tw), d, s), fname


def test_a_rotation_off_by_1e_4_rad_fails():
    for fi, (fname, _, _) in enumerate(R.FRAMES):
        seen = 0
        for name, d, s in R.cases(fi):
            if name in R.GENERIC_500:
                _, _, Ro, to = R.optimum(d, s)
                T = R.pack(Ro, to)
                assert R.passes(T, d, s), (fname, name)
                for angle in (1e-4, -1e-4):
                    assert not R.passes(R.rotated_by(T, angle), d, s), (fname, name, angle)
                seen += 1
        assert seen == len(R.GENERIC_500)


def test_other_defects_fail():
    """a NaN entry, a bottom row that is not 0 0 0 1, a rotation block scaled by 1 + 1e-6"""
    name, d, s = R.cases(0)[7]
    _, _, Ro, to = R.optimum(d, s)
    T = R.pack(Ro, to)
    for i, j, v in ((0, 0, np.nan), (3, 0, 1e-30), (3, 3, np.float32(1) + np.float32(2.0 ** -23))):
        B = T.copy()
        B[i, j] = v
        assert not R.passes(B, d, s), (i, j, v)
    B = T.copy()
    B[:3, :3] *= np.float32(1.000001)
    assert not R.passes(B, d, s)


def test_host_build_of_kabsch_from_sums_over_the_table(exe, tmp_path):
    """every case in every frame through check(); the branch per case; the degenerate and mirrored cases take the SVD fallback"""
    branches = {}
    worst = 0.0
    for fi, (fname, _, _) in enumerate(R.FRAMES):
        table = R.cases(fi)
        got = host_fit(exe, [(d, s) for _, d, s in table], tmp_path)
        for (name, d, s), (T, polar) in zip(table, got):
            f = R.check(T, d, s, f"{fname}/{name}/{'polar' if polar else 'SVD'}")
            if f["scale"] > 0:
                worst = max(worst, f["excess"] / f["scale"])
            branches.setdefault(name, []).append("polar" if polar else "SVD")
    print("branch per case, frames", [f[0] for f in R.FRAMES])
    for name, b in branches.items():
        print(f"  {name}: {b}")
    print("largest excess / scale", worst)
    for name in ("1 pair", "2 pairs", "3 with a repeated point", "3 identical", "3 collinear", "3 mirrored in z", "500 mirrored in z", "500 coplanar",
                 "500 mirrored, 1e-3 noise"):
        assert branches[name][0] == "SVD", (name, branches[name])
    # three pairs are always coplanar about their centroid: sigma has rank <= 2 and EVERY three-pair fit is the fallback's
    assert branches["3 generic"][0] == "SVD"
    assert branches["500 generic"] == ["polar"] * 4 and branches["500 under a rotation by pi"] == ["polar"] * 4
    # no pairs: the identity
    (T, polar), = host_fit(exe, [(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))], tmp_path)
    assert np.array_equal(T, np.eye(4, dtype=np.float32)) and not polar
