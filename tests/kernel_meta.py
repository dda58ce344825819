"""The gfx950 code-object metadata of a built libccmi.so, for the *_resources tests (no GPU
needed): llvm-objdump --offloading unbundles the code object, llvm-readelf --notes prints its
kernel records, c++filt demangles the names.  fmt_kernel() finds a kernel of the formatted output
stage (dec_out.hip), check_fmt_kernel() asserts what all of them keep."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

LIB = Path(__file__).resolve().parents[1] / "cool-chic_amd" / "lib" / "libccmi.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")
KEYS = "vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size"
TYPES = ("float", "F16", "Bf16")

# the geometries of dec_out.hip, as the demangled kernel names spell them
GEOMETRY = {"plain": "Plain", "resize": "Resize<false>", "cubic": "Resize<true>", "warp": "Warp<false, false>",
            "wcubic": "Warp<true, false>", "pwarp": "Warp<false, true>", "pwcubic": "Warp<true, true>"}
# form -> the kernel template: the typed forms without and with colour ops, the statistics pass,
# a resize's horizontal pass
FORMS = {"plain": "dec_fmt", "col": "dec_fmt_col", "stat": "dec_fmt_stat", "h": "dec_resize_h"}


def metadata(lib, tmp_path):
    """{demangled kernel name: {the KEYS}} of lib, unbundled in tmp_path.  Skips the test where the
    library or the ROCm llvm tools are absent."""
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


def fmt_kernel(meta, geometry, form, elem=None, table=False):
    """(demangled name, record) of the ONE kernel of the formatted output stage that is `form` (a key
    of FORMS) of `geometry` (a key of GEOMETRY) for element type `elem` (one of TYPES; None for the
    forms without one: "stat" and "h"), per frame or, table, of a tail group."""
    assert (elem is None) == (form in ("stat", "h")), (form, elem)
    if form == "h":  # the kernel of a tail group is a template of its own
        want = "dec_resize_h%s<%s>" % ("_batch" if table else "", {"resize": "false", "cubic": "true"}[geometry])
    else:  # the template's arguments: geometry, element type, table, then what the launch passes besides
        want = "%s<%s" % (FORMS[form], ", ".join([GEOMETRY[geometry]] + [elem] * bool(elem) + ["true" if table else "false"]))
    pattern = r"(?<![\w:])" + re.escape(want) + (r"\(" if form == "h" else "[,>]")
    hits = [d for d in meta if re.search(pattern, d.replace("ccmi::", "").replace("(anonymous namespace)::", ""))]
    assert len(hits) == 1, (geometry, form, elem, table, hits)
    return hits[0], meta[hits[0]]


def waves(vgprs):
    """waves per SIMD of a wave64 kernel on gfx950: 512 VGPRs a lane, granules of 8, at most 8 waves"""
    return min(8, 512 // (-(-vgprs // 8) * 8))


def check_fmt_kernel(d, v, max_vgprs, lines):
    """what every kernel of the formatted output stage keeps: no scratch, no spill, no LDS, at most
    max_vgprs VGPRs; appends the kernel's line to `lines`"""
    lines.append("%s: %s, %d waves" % (re.sub(r"\(.*", "", d.replace("ccmi::(anonymous namespace)::", ""))[:100], v,
                                      waves(v.get("vgpr_count", 512))))
    for key in KEYS.split("|"):
        assert key in v or key.endswith("spill_count"), lines[-1]
    assert v["private_segment_fixed_size"] == 0, lines[-1]
    assert v.get("vgpr_spill_count", 0) == 0, lines[-1]
    assert v.get("sgpr_spill_count", 0) == 0, lines[-1]
    assert v["group_segment_fixed_size"] == 0, lines[-1]
    assert v["vgpr_count"] <= max_vgprs, lines[-1]
