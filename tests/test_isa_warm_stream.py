"""CPU: what the warm-started iteration's streaming loop (k_warm<., 2>: the record-reading form) must keep in
the code hipcc generates for gfx950 -- properties a later edit loses without any test of results noticing:

  * no scratch and at most 128 VGPRs (four blocks per CU);
  * the record loads of the loop (12-byte source point, 16-byte {match, key}, 12-byte normal; the first 12 bytes of the symmetric
    form's source normal) carry the non-temporal policy bit -- a 400 MB stream re-read every iteration must not allocate in the caches;
  * none of the loop's waits is vmcnt(0): a wait for one register set leaves the other set's loads in flight.

warm.hip is compiled to assembly with the flags of cilantro_amd/build.py; skipped where hipcc is absent."""
import os
import re
import subprocess

import pytest

from cilantro_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = os.path.join(ROOT, "cilantro_amd", "csrc", "warm.hip")
REC2 = re.compile(r"^_ZN6cilhip6k_warmILi(\d+)ELi2ELb([01])EEEvNS_8IterArgsE$")
MAX_VGPRS = 128      # __launch_bounds__(256, 4): 512 registers per SIMD lane / 4 waves

pytestmark = pytest.mark.skipif(not os.path.exists(build.HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / "warm.s")
    cmd = [build.HIPCC] + build.FLAGS + build.EXTRA_FLAGS.get("warm.hip", []) + ["-S", "--cuda-device-only", WARM, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return open(out).read()


def rec2_kernels(txt):
    """{symbol: body} of the k_warm<ACC, 2, SYM> instantiations"""
    out = {}
    for m in re.finditer(r"^(_ZN6cilhip6k_warm\w+):[^\n]*\n(.*?)^\.Lfunc_end", txt, re.S | re.M):
        if REC2.match(m.group(1)):
            out[m.group(1)] = m.group(2)
    return out


def metadata(txt, sym):
    """the kernel's entry of the amdhsa.kernels metadata as {key: value}"""
    for ent in re.split(r"^  - \.", txt[txt.index("amdhsa.kernels:"):], flags=re.M)[1:]:
        kv = dict(re.findall(r"^\s*\.?(\w+):\s+(\S+)\s*$", "." + ent, re.M))
        if kv.get("name") == sym:
            return kv
    raise AssertionError(f"no metadata for {sym}")


def streaming_loop(body):
    """The instructions of the streaming loop: the smallest backward-branch region (label .. branch to it) that holds the loads of both
    register sets (each: one 16-byte record, at least one 12-byte load) and matrix-core instructions -- the loop over the rounds
    (the loop around it also holds the pipeline fill and the list search)."""
    lines = [l.strip() for l in body.splitlines()]
    label_at = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"(\.LBB\d+_\d+):", l))}
    best = None      # (length, head, index of the branch)
    back = []
    for i, l in enumerate(lines):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if not m or label_at.get(m.group(1), i + 1) > i:
            continue
        head = label_at[m.group(1)]
        back.append((head, i))
        region = lines[head:i + 1]
        n3 = sum(x.startswith("global_load_dwordx3") for x in region)
        n4 = sum(x.startswith("global_load_dwordx4") for x in region)
        if n3 >= 2 and n4 >= 2 and any(x.startswith("v_mfma") for x in region):      # both register sets' loads
            if best is None or len(region) < best[0]:
                best = (len(region), head, i)
    assert best is not None, "no loop with two sets of record loads and v_mfma found"
    # (the loop has several latches: up to the LAST branch back to that head)
    return lines[best[1]:max(i for h, i in back if h == best[1]) + 1]


def test_every_rec2_instantiation_is_there(listing):
    ks = rec2_kernels(listing)
    # IM_KABSCH, IM_PLANE, IM_POINT, IM_BOTH, IM_AFFC, IM_AFFP, and the symmetric objective of the two plane-term forms
    assert {(int(REC2.match(k).group(1)), REC2.match(k).group(2)) for k in ks} >= {(1, "0"), (2, "0"), (3, "0"), (4, "0"), (8, "0"), (9, "0"), (2, "1"), (4, "1")}


def test_no_scratch_and_four_blocks_per_cu(listing):
    for sym in rec2_kernels(listing):
        md = metadata(listing, sym)
        assert int(md["private_segment_fixed_size"]) == 0, (sym, md["private_segment_fixed_size"])
        assert int(md["vgpr_count"]) <= MAX_VGPRS, (sym, md["vgpr_count"])
        assert int(md.get("vgpr_spill_count", 0)) == 0, (sym, md.get("vgpr_spill_count"))


def test_record_loads_are_non_temporal(listing):
    for sym, body in rec2_kernels(listing).items():
        acc, symm = int(REC2.match(sym).group(1)), REC2.match(sym).group(2) == "1"
        loop = streaming_loop(body)
        loads = [l for l in loop if re.match(r"global_load_dwordx[34]\b", l)]
        per_set = 2 + (1 if acc in (2, 4, 8) else 0) + (1 if symm else 0)      # source point, record, [normal: FusedZ::needs_normal], [source normal]
        assert len(loads) >= 2 * per_set, (sym, loads)
        for l in loads:
            assert re.search(r"\bnt\b", l), (sym, l)


def test_no_wait_drains_the_prefetches(listing):
    for sym, body in rec2_kernels(listing).items():
        waits = [l for l in streaming_loop(body) if l.startswith("s_waitcnt") and "vmcnt" in l]
        assert waits, sym
        for l in waits:
            assert not re.search(r"vmcnt\(0\)", l), (sym, l)
