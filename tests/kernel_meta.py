"""The gfx950 code-object metadata of a built libccmi.so, for the *_resources tests (no GPU
needed): llvm-objdump --offloading unbundles the code object, llvm-readelf --notes prints its
kernel records, c++filt demangles the names."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

LIB = Path(__file__).resolve().parents[1] / "cool-chic_amd" / "lib" / "libccmi.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")


def metadata(lib, tmp_path):
    """{demangled kernel name: {vgpr_count, vgpr_spill_count, sgpr_spill_count,
    private_segment_fixed_size}} of lib, unbundled in tmp_path.  Skips the test where the library
    or the ROCm llvm tools are absent."""
    objdump, readelf = LLVM / "llvm-objdump", LLVM / "llvm-readelf"
    if not (Path(lib).exists() and objdump.exists() and readelf.exists()):
        pytest.skip("libccmi.so or the ROCm llvm tools are absent")
    copy = tmp_path / "libccmi.so"
    shutil.copy(lib, copy)
    subprocess.run([str(objdump), "--offloading", str(copy)], cwd=tmp_path, check=True, capture_output=True)
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
