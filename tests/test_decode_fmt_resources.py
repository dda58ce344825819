"""Register / scratch use of the formatted-output kernels (dec_output_fmt<T>, the per-frame
cropping form, and dec_output_fmt_batch<T>, the tail groups' form), read from the gfx950
code-object metadata of the built libccmi.so as tests/test_kernel_resources.py does (no GPU
needed).  The stage keeps 4 pixels x 3 channels per thread in registers and must use no
scratch and spill nothing.

As built: 35 VGPRs for each of the six instantiations (float, F16, Bf16 x the two forms);
the planar float32 output kernel it stands in for has 29."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "cool-chic_amd" / "lib" / "libccmi.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")
FORMS = ("dec_output_fmt<", "dec_output_fmt_batch<")
TYPES = ("float", "F16", "Bf16")
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


def test_formatted_output_kernels_use_no_scratch(tmp_path):
    meta = _metadata(tmp_path)
    lines = []
    for form in FORMS:
        for t in TYPES:
            hits = [(d, v) for d, v in meta.items() if form in d and re.search(r"<(\w+::)*(\(anonymous namespace\)::)?%s>" % t, d)]
            assert len(hits) == 1, (form, t, [d for d, _ in hits])
            d, v = hits[0]
            lines.append(f"{d[:110]}: {v}")
            assert "vgpr_count" in v and "private_segment_fixed_size" in v, lines[-1]
            assert v["private_segment_fixed_size"] == 0, lines[-1]
            assert v.get("vgpr_spill_count", 0) == 0, lines[-1]
            assert v.get("sgpr_spill_count", 0) == 0, lines[-1]
            assert v["vgpr_count"] <= MAX_VGPRS, lines[-1]
    print("\n".join(lines))
