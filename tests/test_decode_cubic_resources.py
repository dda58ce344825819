"""Register, scratch and LDS use of the bicubic output kernels, read from the gfx950 code-object
metadata of the built libccmi.so in the form of tests/test_decode_resample_resources.py (no GPU
needed): dec_cubic_h, dec_cubic_v<T>, dec_wcubic<T>, their _col and _stat forms, each per frame and
_batch -- 30 kernels.  Every one must be there exactly once, use no scratch, spill nothing and use no
LDS.  128 VGPRs is the hard bound (4 waves per SIMD) and is asserted; 64 (8 waves) is the aim: the
resize kernels and the warp's statistics pass meet it (they ask the compiler for 8 waves, which it
grants without a spill), the typed warp kernels do not (at 64 they spill 13 to 60 registers, so they
are left to the allocator: 5 to 7 waves) and are printed.  VGPRs as built (per frame / _batch):
    dec_cubic_h                    36 / 36
    dec_cubic_v<float>             58 / 58   <F16|Bf16> 60 / 60   _col 60 / 60   _stat 60 / 60
    dec_wcubic_stat                64 / 64
    dec_wcubic<float>              83 / 90   _col 91 / 91
    dec_wcubic<F16|Bf16>           72 / 82   _col 80 / 83
kernel_meta.metadata() does not read the LDS size, so this file reads the notes itself."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from kernel_meta import LIB, LLVM

TYPES = ("float", "F16", "Bf16")
PLAIN = ("dec_cubic_h(", "dec_cubic_h_batch(", "dec_cubic_v_stat(", "dec_cubic_v_stat_batch(", "dec_wcubic_stat(",
         "dec_wcubic_stat_batch(")
TYPED = ("dec_cubic_v<", "dec_cubic_v_batch<", "dec_cubic_v_col<", "dec_cubic_v_col_batch<", "dec_wcubic<",
         "dec_wcubic_batch<", "dec_wcubic_col<", "dec_wcubic_col_batch<")
MAX_VGPRS = 128  # the hard bound
AIM_VGPRS = 64   # 8 waves per SIMD
KEYS = "vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size"


def _metadata(lib, tmp_path):
    """{demangled kernel name: {the KEYS}} of lib's gfx950 code object, as kernel_meta.metadata() with
    group_segment_fixed_size (the LDS bytes) added."""
    objdump, readelf = LLVM / "llvm-objdump", LLVM / "llvm-readelf"
    if not (Path(lib).exists() and objdump.exists() and readelf.exists()):
        pytest.skip("libccmi.so or the ROCm llvm tools are absent")
    copy = tmp_path / "libccmi.so"
    shutil.copy(lib, copy)
    subprocess.run([str(objdump), "--offloading", str(copy)], cwd=tmp_path, check=True, capture_output=True)
    text = "".join(subprocess.run([str(readelf), "--notes", str(f)], capture_output=True, text=True).stdout
                   for f in sorted(tmp_path.glob("libccmi.so.*gfx950")))
    out, name, pending = {}, None, {}
    for line in text.splitlines():  # a record's keys are sorted, so .group_segment_fixed_size precedes .name
        if re.match(r"\s+- \.", line):
            pending, name = {}, None
            line = line.replace("- ", "  ", 1)
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
            out[name] = pending
            continue
        m = re.match(r"\s+\.(%s):\s+(\d+)" % KEYS, line)
        if m:
            pending[m.group(1)] = int(m.group(2))
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {d: out[n] for n, d in zip(names, dem)}


def test_cubic_kernels_use_no_scratch_no_lds_and_fit_the_registers(tmp_path):
    meta = _metadata(LIB, tmp_path)
    wanted = [(form, None) for form in PLAIN] + [(form, t) for form in TYPED for t in TYPES]
    assert len(wanted) == 30
    lines, over = [], []
    for form, t in wanted:
        hits = [(d, v) for d, v in meta.items() if form in d and
                (t is None or re.search(r"<(\w+::)*(\(anonymous namespace\)::)?%s>" % t, d))]
        assert len(hits) == 1, (form, t, [d for d, _ in hits])
        d, v = hits[0]
        lines.append(f"{d[:96]}: {v}")
        for key in KEYS.split("|"):
            assert key in v or key.endswith("spill_count"), lines[-1]
        assert v["private_segment_fixed_size"] == 0, lines[-1]
        assert v.get("vgpr_spill_count", 0) == 0, lines[-1]
        assert v.get("sgpr_spill_count", 0) == 0, lines[-1]
        assert v["group_segment_fixed_size"] == 0, lines[-1]
        assert v["vgpr_count"] <= MAX_VGPRS, lines[-1]
        if v["vgpr_count"] > AIM_VGPRS:
            over.append(lines[-1])
    print("\n".join(lines))
    print("above %d VGPRs: %s" % (AIM_VGPRS, over or "none"))
