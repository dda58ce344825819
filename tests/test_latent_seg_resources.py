"""Register / scratch use of the segmented latent store's kernels (dec_lat_seg_width,
dec_lat_seg_scan, dec_lat_seg_pack, dec_lat_unpack_seg), read from the gfx950 code-object
metadata of the built libccmi.so in the form of tests/test_decode_resample_resources.py (no GPU
needed).  They are memory-bound copies: no kernel may use scratch or spill, and each fits 8
waves per SIMD.  The typed pack / unpack kernels of the other storage forms are still there."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "cool-chic_amd" / "lib" / "libccmi.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")
NEW = ("dec_lat_seg_width(", "dec_lat_seg_scan(", "dec_lat_seg_pack(", "dec_lat_unpack_seg(")
TYPED = ("dec_lat_pack<", "dec_lat_unpack<")
TYPES = ("signed char", "short", "int")
MAX_VGPRS = 64  # 8 waves per SIMD


def _metadata(tmp_path):
    objdump, readelf = LLVM / "llvm-objdump", LLVM / "llvm-readelf"
    if not (LIB.exists() and objdump.exists() and readelf.exists()):
        pytest.skip("libccmi.so or the ROCm llvm tools are absent")
    lib = tmp_path / "libccmi.so"
    shutil.copy(LIB, lib)
    subprocess.run([str(objdump), "--offloading", str(lib)], cwd=tmp_path, check=True, capture_output=True)
    text = "".join(subprocess.run([str(readelf), "--notes", str(f)], capture_output=True, text=True).stdout
                   for f in sorted(tmp_path.glob("libccmi.so.*gfx950")))
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.match(r"\s+\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {d: out[n] for n, d in zip(names, dem)}


def _lean(d, v):
    line = f"{d[:110]}: {v}"
    assert "vgpr_count" in v and "private_segment_fixed_size" in v, line
    assert v["private_segment_fixed_size"] == 0, line
    assert v.get("vgpr_spill_count", 0) == 0, line
    assert v.get("sgpr_spill_count", 0) == 0, line
    assert v["vgpr_count"] <= MAX_VGPRS, line
    return line


def test_segmented_store_kernels_use_no_scratch(tmp_path):
    meta = _metadata(tmp_path)
    lines = []
    for form in NEW:
        hits = [(d, v) for d, v in meta.items() if form in d]
        assert len(hits) == 1, (form, [d for d, _ in hits])
        lines.append(_lean(*hits[0]))
    print("\n".join(lines))


def test_typed_pack_and_unpack_are_still_there(tmp_path):
    meta = _metadata(tmp_path)
    for form in TYPED:
        for t in TYPES:
            hits = [d for d in meta if form in d and re.search(r"<%s>" % t, d)]
            assert len(hits) == 1, (form, t, hits)
