"""A/B of the compact latent store (LatentStore.compact: per-segment bit widths) and of one
store object over many (LatentStore.concat) against the int16 store they are made from, on one
GPU, in one process, alternating, on 960 class-E frames (the 15 committed 1280x720 streams x 64)
and 320 class-B frames (the 5 committed 1920x1080 streams x 64), in the form of
tools/decode_latents_ab.py.  Per set:
  bytes per stream of the store at int16 / int8 (ccmi_latents_plan) and in the segmented form
  (measured by the compaction), and what the compaction's workspace takes;
  MEAS  ccmi_latents_compact_measure   (width pass + offset scan, sizes read back)
  COMP  ccmi_latents_compact           (the same again, then the pack)
  the render_model of profiles/decode_model_ab.txt (256 x 256 regions at seeded random even
  origins, RGB, ImageNet mean / std, bfloat16, NCHW) from
  M16   the int16 store
  MSEG  its compaction
  MCAT  a concat of 8 compacted chunks (each built, compacted and its int16 store dropped)
  with the unpack stage and the tail of decode.last_timing() and the tail groups of each.
Warm-up rounds of every leg, then `--reps` (>= 7) alternating repetitions, each ended by a
device synchronise; median [min .. max].  The three renders' last results are compared.

--mode parent measures render(float32) of an int16 store through the C ABI
(ccmi_latents_decode / ccmi_latents_render, whole call, caller-owned workspace and outputs) with
two libraries loaded side by side in this process, alternating: this tree's libccmi.so and one
built from the parent commit (--parent-lib).  The rule of profiles/decode_split_ab.txt: the new
library's median lies inside the parent's own spread over the runs (run the mode twice).
The report is appended to --out."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "cool-chic_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ccmi import decode, encode  # noqa: E402

SIDE = 256
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CHUNKS = 8
P, I, Z = C.c_void_p, C.c_int, C.c_size_t


def _stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def _fmt(e):
    return f"{e['median']:8.2f} [{e['min']:8.2f} .. {e['max']:8.2f}]"


def _rois(n, H, W):
    rng = np.random.default_rng(17)
    return [(2 * int(rng.integers(0, (W - SIDE) // 2 + 1)), 2 * int(rng.integers(0, (H - SIDE) // 2 + 1)), SIDE, SIDE)
            for _ in range(n)]


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def run_set(cls, copies, reps, warmup):
    files = sorted((ROOT / "tests/golden/cool").glob(f"{cls}-*.cool"))
    streams = [f.read_bytes() for _ in range(copies) for f in files]
    desc = encode.parse(streams[0]).desc
    H, W, n = desc.h, desc.w, len(streams)
    rois = _rois(n, H, W)
    L = decode._bind()
    keep, sp, ln = decode._marshal(streams)
    planned = {}
    for name, t in (("int8", decode.LATENT_I8), ("int16", decode.LATENT_I16)):
        tot, ws = C.c_size_t(0), C.c_size_t(0)
        decode.check(L.ccmi_latents_plan(sp, ln, n, t, C.byref(tot), None, C.byref(ws)))
        planned[name] = tot.value / n
    del keep, sp, ln
    s16 = decode.LatentStore(streams, dtype=torch.int16)
    # the compaction calls themselves, workspace and store allocated outside the timed part
    bound, nws, exact = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    decode.check(L.ccmi_latents_compact_plan(s16._handle(), C.byref(bound), C.byref(nws)))
    cws = torch.empty(max(nws.value, 256), dtype=torch.uint8, device="cuda")
    hs = torch.cuda.current_stream().cuda_stream
    decode.check(L.ccmi_latents_compact_measure(s16._handle(), cws.data_ptr(), cws.numel(), hs, C.byref(exact), None))
    cstore = torch.empty(max(exact.value, 256), dtype=torch.uint8, device="cuda")
    t_meas, t_comp = [], []

    def measure():
        decode.check(L.ccmi_latents_compact_measure(s16._handle(), cws.data_ptr(), cws.numel(), hs, C.byref(exact), None))

    def compact():
        h = C.c_void_p(None)
        decode.check(L.ccmi_latents_compact(s16._handle(), cstore.data_ptr(), cstore.numel(), cws.data_ptr(), cws.numel(), hs,
                                            C.byref(h)))
        L.ccmi_latents_free(h)
    for it in range(warmup + reps):
        _, a = _timed(measure)
        _, b = _timed(compact)
        if it >= warmup:
            t_meas.append(a)
            t_comp.append(b)
    del cstore, cws
    sseg = s16.compact()
    per = (n + CHUNKS - 1) // CHUNKS
    parts = []
    for c in range(CHUNKS):
        part = decode.LatentStore(streams[c * per: (c + 1) * per], dtype=torch.int16)
        parts.append(part.compact())
        part.close()
    scat = decode.LatentStore.concat(parts)
    for p in parts:
        p.close()
    del streams
    stores = {"M16": s16, "MSEG": sseg, "MCAT": scat}
    need = s16.render_geometry(roi=rois, dtype=torch.float32)[1]
    assert all(st.render_geometry(roi=rois, dtype=torch.float32)[1] == need for st in stores.values())
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
    rec = {k: {"wall_ms": [], "unpack_ms": [], "tail_ms": []} for k in stores}
    last, groups = {}, {}
    for it in range(warmup + reps):
        for k, st in stores.items():
            last[k] = None
            last[k], dt = _timed(lambda st=st: st.render_model(roi=rois, mean=MEAN, std=STD, dtype=torch.bfloat16, workspace=ws))
            tm = decode.last_timing()
            groups[k] = decode.last_tail_groups()
            if it >= warmup:
                rec[k]["wall_ms"].append(dt)
                rec[k]["unpack_ms"].append(tm["arm_cabac"])
                rec[k]["tail_ms"].append(tm["ups_syn_out"])
    same = {k: bool(torch.equal(last[k].view(torch.int16), last["M16"].view(torch.int16))) for k in ("MSEG", "MCAT")}
    out = {"set": f"class {cls}: {len(files)} streams x {copies} = {n} frames of {W}x{H}", "frames": n,
           "bytes_per_stream": {"int16": planned["int16"], "int8": planned["int8"], "seg": sseg.nbytes / n,
                                "seg_concat": scat.nbytes / n, "seg_bound": bound.value / n},
           "compact_workspace_bytes": nws.value, "measure_ms": _stat(t_meas), "compact_ms": _stat(t_comp),
           "render_workspace_bytes": need, "legs": {k: {s: _stat(v) for s, v in rec[k].items()} for k in stores},
           "tail_groups": groups, "equal_to_int16": same, "dtypes": {k: str(st.dtype) for k, st in stores.items()}}
    for st in stores.values():
        st.close()
    return out


class CLib:
    """One libccmi.so through ctypes: an int16 store of `streams` and its float32 render."""

    def __init__(self, path, streams, rois):
        L = self.L = C.CDLL(str(path))
        L.ccmi_latents_plan.argtypes = [P, P, I, I, P, P, P]
        L.ccmi_latents_decode.argtypes = [P, P, I, I, P, Z, P, Z, P, P]
        L.ccmi_latents_render_plan.argtypes = [P, P, I, P, I, I, I, P, P, P]
        L.ccmi_latents_render.argtypes = [P, P, I, P, P, P, I, I, I, P, Z, P]
        L.ccmi_last_error.restype = C.c_char_p
        n = self.n = len(streams)
        keep, sp, ln = decode._marshal(streams)
        tot, nws = C.c_size_t(0), C.c_size_t(0)
        self.check(L.ccmi_latents_plan(sp, ln, n, decode.LATENT_I16, C.byref(tot), None, C.byref(nws)))
        self.store = torch.empty(tot.value, dtype=torch.uint8, device="cuda")
        bws = torch.empty(nws.value, dtype=torch.uint8, device="cuda")
        self.h = C.c_void_p(None)
        self.check(L.ccmi_latents_decode(sp, ln, n, decode.LATENT_I16, self.store.data_ptr(), tot.value, bws.data_ptr(),
                                         bws.numel(), None, C.byref(self.h)))
        self.rects = (decode.Rect * n)(*[decode.Rect(*r) for r in rois])
        geom, need = (decode.FrameGeom * n)(), C.c_size_t(0)
        self.check(L.ccmi_latents_render_plan(self.h, None, n, self.rects, 0, 0, decode.SAMPLE_F32, geom, None, C.byref(need)))
        self.ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
        elems = [g.elems for g in geom]
        self.out = torch.empty(sum(elems), dtype=torch.float32, device="cuda")
        at = np.concatenate([[0], np.cumsum(elems)])
        self.op = (C.c_void_p * n)(*[self.out.data_ptr() + 4 * int(a) for a in at[:-1]])
        self.cap = (C.c_size_t * n)(*[4 * e for e in elems])

    def check(self, rc):
        if rc:
            raise RuntimeError(self.L.ccmi_last_error().decode())

    def render(self):
        self.check(self.L.ccmi_latents_render(self.h, None, self.n, self.rects, self.op, self.cap, decode.SAMPLE_F32, 0, 0,
                                              self.ws.data_ptr(), self.ws.numel(), None))


def run_parent(cls, copies, reps, warmup, parent_lib):
    files = sorted((ROOT / "tests/golden/cool").glob(f"{cls}-*.cool"))
    streams = [f.read_bytes() for _ in range(copies) for f in files]
    desc = encode.parse(streams[0]).desc
    n = len(streams)
    rois = _rois(n, desc.h, desc.w)
    libs = {"parent": CLib(parent_lib, streams, rois), "new": CLib(decode.lib()._name, streams, rois)}
    rec = {k: [] for k in libs}
    for it in range(warmup + reps):
        for k, lib in libs.items():
            _, dt = _timed(lib.render)
            if it >= warmup:
                rec[k].append(dt)
    same = bool(torch.equal(libs["parent"].out, libs["new"].out))
    return {"set": f"class {cls}: {n} frames of {desc.w}x{desc.h}", "legs": {k: _stat(v) for k, v in rec.items()},
            "equal": same}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=("compact", "parent"), default="compact")
    ap.add_argument("--parent-lib", default="", help="--mode parent: a libccmi.so built from the parent commit")
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", default="E,B")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "decode_compact_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_compact_ab: no HIP device (this is a GPU measurement)")
    if a.reps < 7:
        sys.exit("decode_compact_ab: at least 7 repetitions")
    if a.mode == "parent" and not Path(a.parent_lib).is_file():
        sys.exit("decode_compact_ab: --mode parent needs --parent-lib")
    head = ("compact latent store A/B: render_model from an int16 store, its compaction and a concat of compacted chunks, alternating"
            if a.mode == "compact" else "render(float32) of an int16 store through the C ABI: the parent commit's library against this tree's, alternating")
    lines = [head, f"device: {torch.cuda.get_device_name(0)}; one process; median [min .. max] of {a.reps} repetitions "
                   f"after {a.warmup} warm-up rounds; {SIDE}x{SIDE} regions at random even origins", ""]
    for cls in a.sets.split(","):
        if a.mode == "parent":
            r = run_parent(cls, a.copies, a.reps, a.warmup, a.parent_lib)
            lines.append(r["set"])
            for k, e in r["legs"].items():
                lines.append(f"  {k:6s} render(float32) whole call {_fmt(e)} ms")
            p, q = r["legs"]["parent"], r["legs"]["new"]
            lines.append(f"  new median {q['median']:.3f} against the parent's range [{p['min']:.3f} .. {p['max']:.3f}]: "
                         f"{'inside' if q['median'] <= p['max'] else 'ABOVE'}; outputs equal: {r['equal']}")
        else:
            r = run_set(cls, a.copies, a.reps, a.warmup)
            lines.append(r["set"])
            b = r["bytes_per_stream"]
            lines.append(f"  store bytes per stream (GPU, measured): int16 {b['int16']:.0f}, int8 {b['int8']:.0f}, seg {b['seg']:.0f} "
                         f"({b['seg'] / b['int16']:.3f} of int16; in {CHUNKS} chunks {b['seg_concat']:.0f}; 32-bit bound {b['seg_bound']:.0f}); "
                         f"compaction workspace {r['compact_workspace_bytes'] / 2**20:.1f} MiB")
            lines.append(f"  MEAS compact_measure {_fmt(r['measure_ms'])} ms   COMP compact {_fmt(r['compact_ms'])} ms")
            for k, e in r["legs"].items():
                lines.append(f"  {k:5s} render_model ({r['dtypes'][k]:>11s}) wall {_fmt(e['wall_ms'])} ms  unpack {_fmt(e['unpack_ms'])}  "
                             f"tail {_fmt(e['tail_ms'])}  tail groups {tuple(r['tail_groups'][k])}")
            lines.append(f"  equal to the int16 store's result, bit for bit: {r['equal_to_int16']}; render workspace "
                         f"{r['render_workspace_bytes'] / 2**20:.1f} MiB for every store")
        lines.append("  json: " + json.dumps(r))
        lines.append("")
    text = "\n".join(lines)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
