"""A/B of reopening a latent store from a file (ccmi_latents_export / ccmi_latents_import,
LatentStore.save / load) against building it again from the coded streams, on one GPU, in one
process, alternating, on 960 class-E frames (the 15 committed 1280x720 streams x 64), in the form
of tools/decode_compact_ab.py.  Legs, each a whole call ended by a device synchronise:
  BUILD  LatentStore(streams, int16) + compact()      what every process pays without a file
  EXPORT ccmi_latents_export of the compact store     into a pinned host buffer, workspace given
  IMPORT ccmi_latents_import of that buffer           from pinned memory, store and workspace given,
         with the upload and the checksum + verify stages of decode.last_timing()
  SAVE / LOAD  LatentStore.save / load through a file in --dir (page cache warm)
and the file's bytes.  The loaded store's render_model (256 x 256 regions, RGB, bfloat16) is compared
with the compact store's, bit for bit.  Warm-up rounds, then `--reps` (>= 7) alternating
repetitions; median [min .. max].  The report is appended to --out."""
import argparse
import ctypes as C
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "cool-chic_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ccmi import decode, encode  # noqa: E402

SIDE = 256
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def _fmt(e):
    return f"{e['median']:8.2f} [{e['min']:8.2f} .. {e['max']:8.2f}]"


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def run_set(cls, copies, reps, warmup, where):
    files = sorted((ROOT / "tests/golden/cool").glob(f"{cls}-*.cool"))
    streams = [f.read_bytes() for _ in range(copies) for f in files]
    desc = encode.parse(streams[0]).desc
    H, W, n = desc.h, desc.w, len(streams)
    rng = np.random.default_rng(17)
    rois = [(2 * int(rng.integers(0, (W - SIDE) // 2 + 1)), 2 * int(rng.integers(0, (H - SIDE) // 2 + 1)), SIDE, SIDE)
            for _ in range(n)]
    L = decode._bind()
    hs = torch.cuda.current_stream().cuda_stream

    def build():
        s16 = decode.LatentStore(streams, dtype=torch.int16)
        seg = s16.compact()
        s16.close()
        return seg
    seg = build()
    nmeta, nfile, nws = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    decode.check(L.ccmi_latents_export_plan(seg._handle(), None, n, C.byref(nmeta), C.byref(nfile), C.byref(nws)))
    host = torch.empty(nfile.value, dtype=torch.uint8, pin_memory=True)
    ews = torch.empty(max(nws.value, 256), dtype=torch.uint8, device="cuda")

    def export():
        decode.check(L.ccmi_latents_export(seg._handle(), None, n, None, host.data_ptr(), host.numel(), ews.data_ptr(),
                                           ews.numel(), hs))
    export()
    meta = bytes(host[: nmeta.value].numpy())
    off, nb, iws = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    decode.check(L.ccmi_latents_import_plan(meta, len(meta), 0, -1, C.byref(off), C.byref(nb), None, C.byref(iws)))
    store = torch.empty(max(nb.value, 256), dtype=torch.uint8, device="cuda")
    ws = torch.empty(max(iws.value, 256), dtype=torch.uint8, device="cuda")

    def imp():
        h = C.c_void_p(None)
        decode.check(L.ccmi_latents_import(meta, len(meta), 0, -1, host.data_ptr() + off.value, nb.value, store.data_ptr(),
                                           store.numel(), ws.data_ptr(), ws.numel(), hs, None, C.byref(h)))
        L.ccmi_latents_free(h)
    path = Path(where) / f"class{cls}.cclat"
    rec = {k: [] for k in ("BUILD", "EXPORT", "IMPORT", "upload", "verify", "SAVE", "LOAD")}
    for it in range(warmup + reps):
        got = {}
        b, got["BUILD"] = _timed(build)
        b.close()
        _, got["EXPORT"] = _timed(export)
        _, got["IMPORT"] = _timed(imp)
        tm = decode.last_timing()
        got["upload"], got["verify"] = tm["upload"], tm["arm_cabac"]
        _, got["SAVE"] = _timed(lambda: seg.save(path))
        ld, got["LOAD"] = _timed(lambda: decode.LatentStore.load(path))
        if it >= warmup:
            for k, v in got.items():
                rec[k].append(v)
        if it + 1 < warmup + reps:
            ld.close()
    kw = dict(roi=rois, mean=MEAN, std=STD, dtype=torch.bfloat16)
    same = bool(torch.equal(seg.render_model(**kw).view(torch.int16), ld.render_model(**kw).view(torch.int16)))
    out = {"set": f"class {cls}: {len(files)} streams x {copies} = {n} frames of {W}x{H}", "frames": n,
           "file_bytes": nfile.value, "meta_bytes": nmeta.value, "export_workspace_bytes": nws.value,
           "import_workspace_bytes": iws.value, "legs": {k: _stat(v) for k, v in rec.items()}, "renders_equal": same}
    path.unlink()
    ld.close()
    seg.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", default="E")
    ap.add_argument("--dir", default=tempfile.gettempdir(), help="where the file of the SAVE / LOAD legs goes")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "decode_store_file_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_store_file_ab: no HIP device (this is a GPU measurement)")
    if a.reps < 7:
        sys.exit("decode_store_file_ab: at least 7 repetitions")
    lines = ["latent store files A/B: build + compact from coded streams against export / import / save / load, alternating",
             f"device: {torch.cuda.get_device_name(0)}; one process; median [min .. max] of {a.reps} repetitions after "
             f"{a.warmup} warm-up rounds", ""]
    for cls in a.sets.split(","):
        r = run_set(cls, a.copies, a.reps, a.warmup, a.dir)
        lines.append(r["set"])
        lines.append(f"  file {r['file_bytes']} bytes ({r['file_bytes'] / r['frames']:.0f} per stream, META {r['meta_bytes']}); "
                     f"workspace export {r['export_workspace_bytes'] / 2**20:.1f} MiB, import "
                     f"{r['import_workspace_bytes'] / 2**10:.1f} KiB")
        for k, e in r["legs"].items():
            lines.append(f"  {k:7s} {_fmt(e)} ms")
        lines.append(f"  the loaded store's render_model equals the compact store's, bit for bit: {r['renders_equal']}")
        lines.append("  json: " + json.dumps(r))
        lines.append("")
    text = "\n".join(lines)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
