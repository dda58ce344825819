"""Register / scratch / LDS use of the filter kernels (dec_filter<T>, dec_filter_batch<T>; T = float, F16,
Bf16), read from the gfx950 code-object metadata of the built libccmi.so in the form of
tests/test_decode_colour_resources.py (no GPU needed).

The radius and the taps are scalars (the taps come from the frame's table entry by scalar loads), the
horizontal result lives in LDS, and a thread keeps its two groups of 4 pixels x 3 channels converted to
the element type: no kernel may use scratch or spill, the static LDS stays under 64 kB, and 64 VGPRs keep
8 waves per SIMD as far as registers go (measured: 44 VGPRs and 41,804 bytes of LDS for all six; the
LDS allows 3 blocks of 4 waves per CU)."""
import re
import subprocess

from kernel_meta import LIB, LLVM, metadata

FORMS = ("dec_filter<", "dec_filter_batch<")
TYPES = ("float", "F16", "Bf16")
MAX_VGPRS = 64        # 8 waves per SIMD
MAX_LDS = 64 * 1024   # static LDS of one block


def _lds(tmp_path):
    """{demangled kernel name: group_segment_fixed_size} of the code object metadata() unbundled in tmp_path"""
    text = "".join(subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(f)], capture_output=True, text=True).stdout
                   for f in sorted(tmp_path.glob("libccmi.so.*gfx950")))
    out, size = {}, None
    for line in text.splitlines():  # a kernel record lists .group_segment_fixed_size before .name
        m = re.match(r"\s+\.group_segment_fixed_size:\s+(\d+)", line)
        if m:
            size = int(m.group(1))
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m and size is not None:
            out[m.group(1)] = size
            size = None
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {d: out[n] for n, d in zip(names, dem)}


def test_filter_kernels_use_no_scratch_and_fit_the_lds(tmp_path):
    meta = metadata(LIB, tmp_path)
    lds = _lds(tmp_path)
    lines = []
    for form in FORMS:
        for t in TYPES:
            hits = [(d, v) for d, v in meta.items() if form in d and
                    re.search(r"%s(\w+::)*(\(anonymous namespace\)::)?%s>" % (re.escape(form), t), d)]
            assert len(hits) == 1, (form, t, [d for d, _ in hits])
            d, v = hits[0]
            lines.append(f"{d[:110]}: {v} lds {lds.get(d)}")
            assert "vgpr_count" in v and "private_segment_fixed_size" in v, lines[-1]
            assert v["private_segment_fixed_size"] == 0, lines[-1]
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, lines[-1]
            assert v["vgpr_count"] <= MAX_VGPRS, lines[-1]
            assert d in lds and 0 < lds[d] <= MAX_LDS, lines[-1]
    print("\n".join(lines))
