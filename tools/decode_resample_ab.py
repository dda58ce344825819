"""A/B of the resampling output stage (LatentStore.render_model(size=...): RandomResizedCrop-style
regions of different sizes resampled to one size in the decoder's output stage, one batched tail)
against the path it replaces, on one GPU, in one process, legs alternating, on the bench's
`bitexact_decode` set (the 15 committed class-E 1280x720 streams x 64 = 960 frames) held in a
LatentStore.  Regions: area U(0.08, 1) of the frame, aspect log-uniform in [3/4, 4/3], origin
uniform, rects rounded to even (seeded); output 224 x 224, RGB, ImageNet mean / std, bfloat16,
a seeded random mirror per frame.
  N   store.render_model(roi=..., size=(224, 224), mean=..., std=..., dtype=bfloat16, mirror=...)
  C   the composed path: store.render_model(dtype=float32) once per distinct region size, then per
      sample torch.nn.functional.interpolate(mode="bilinear", antialias=True), * scale + bias,
      the cast to bfloat16 and the flip, written into one [n, 3, 224, 224] tensor.
Warm-up rounds of both legs, then `--reps` (>= 7) alternating wall-clock repetitions, each ended by
a device synchronise.  Reported per leg: median and range of the time per call, the peak of torch's
allocated bytes above what was allocated before the leg (store and render workspaces are the
caller's, allocated before), and the batched tail groups / per-frame tails the leg launched
(decode.last_tail_groups(), summed over the leg's calls).  The two results are compared: N
follows the contract's float32 order, torch's interpolate its own, so they differ in rounding
(counted and bounded, not asserted).

--mode regress: the unchanged call, store.render_model(256 x 256 regions, no size), through the
C ABI of two libraries in one process, alternating: --parent (a libccmi.so built from the parent
commit) and the tree's own, in the element type of --dtype (bfloat16, float32 or float16).  Each
library builds its own store and workspace.  The rule is that of
profiles/decode_split_ab.txt, per run of this tool: reference = the lowest of the parent's
per-block medians, allowance = their spread; the new library's median of block medians must not
exceed reference + allowance.  The repetitions are split into three blocks per library for this.

Run each mode twice; the report is appended to --out."""
import argparse
import ctypes as C
import math
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "cool-chic_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ccmi import decode  # noqa: E402

OUT = (224, 224)
SIDE = 256
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
W, H = 1280, 720


def _stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def _fmt_stat(v, unit=1.0):
    e = _stat(v)
    return f"{e['median'] / unit:9.2f} [{e['min'] / unit:9.2f} .. {e['max'] / unit:9.2f}]"


def rrc_rects(n, rng):
    """RandomResizedCrop geometry (torchvision's sampling), rounded to even, inside the frame."""
    out = []
    for _ in range(n):
        for _ in range(10):
            area = W * H * rng.uniform(0.08, 1.0)
            ratio = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
            w, h = int(round(math.sqrt(area * ratio))) & ~1, int(round(math.sqrt(area / ratio))) & ~1
            if 2 <= w <= W and 2 <= h <= H:
                break
        else:
            w, h = H, H
        out.append((2 * int(rng.integers(0, (W - w) // 2 + 1)), 2 * int(rng.integers(0, (H - h) // 2 + 1)), w, h))
    return out


def mode_resample(a, streams):
    n = len(streams)
    rng = np.random.default_rng(17)
    rects = rrc_rects(n, rng)
    mirror = [bool(v) for v in rng.integers(0, 2, n)]
    store = decode.LatentStore(streams, dtype=torch.int16)
    scale = torch.tensor([float(np.float32(1.0 / s)) for s in STD], device="cuda").view(1, 3, 1, 1)
    bias = torch.tensor([float(np.float32(-m / s)) for m, s in zip(MEAN, STD)], device="cuda").view(1, 3, 1, 1)
    by_size = {}
    for j, r in enumerate(rects):
        by_size.setdefault((r[3], r[2]), []).append(j)
    need_n = store.render_model_workspace_bytes(roi=rects, size=OUT)
    need_c = max(store.render_model_workspace_bytes(index=js, roi=[rects[j] for j in js]) for js in by_size.values())
    ws_n = torch.empty(max(need_n, 256), dtype=torch.uint8, device="cuda")
    ws_c = torch.empty(max(need_c, 256), dtype=torch.uint8, device="cuda")

    def leg_new():
        out = store.render_model(roi=rects, size=OUT, mean=MEAN, std=STD, dtype=torch.bfloat16, mirror=mirror, workspace=ws_n)
        return out, decode.last_tail_groups()

    def leg_composed():
        out = torch.empty(n, 3, *OUT, dtype=torch.bfloat16, device="cuda")
        groups = [0, 0]
        for js in by_size.values():
            x = store.render_model(index=js, roi=[rects[j] for j in js], dtype=torch.float32, workspace=ws_c)
            g = decode.last_tail_groups()
            groups[0] += g[0]
            groups[1] += g[1]
            y = torch.nn.functional.interpolate(x, size=OUT, mode="bilinear", antialias=True, align_corners=False)
            y = (y * scale + bias).to(torch.bfloat16)
            for k, j in enumerate(js):
                out[j] = y[k].flip(-1) if mirror[j] else y[k]
        return out, tuple(groups)

    legs = {"N": leg_new, "C": leg_composed}
    rec = {k: {"wall": [], "peak": []} for k in legs}
    last, groups = {}, {}
    for it in range(a.warmup + a.reps):
        for k, fn in legs.items():
            last[k] = None
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            last[k], groups[k] = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if it >= a.warmup:
                rec[k]["wall"].append(1e3 * dt)
                rec[k]["peak"].append(torch.cuda.max_memory_allocated() - base)
    area = [r[2] * r[3] / (W * H) for r in rects]
    names = {"N": "N  render_model(size=(224, 224))            ", "C": "C  render_model(float32) + interpolate      "}
    lines = ["resampling output stage A/B: LatentStore.render_model(size=...) against render_model(float32) per region size "
             "+ torch interpolate(antialias=True), alternating",
             f"device: {torch.cuda.get_device_name(0)}; one process; {n} class-E frames of {W}x{H}; RandomResizedCrop regions "
             f"(area {min(area):.2f} .. {max(area):.2f} of the frame, mean {sum(area) / n:.2f}; {len(by_size)} distinct sizes) "
             f"-> {OUT[0]}x{OUT[1]} bf16 RGB normalised, random mirror; median [min .. max] of {a.reps} repetitions after "
             f"{a.warmup} warm-up rounds; workspaces (caller-owned, not in the peaks): N {need_n / 2**20:.0f} MiB, "
             f"C {need_c / 2**20:.0f} MiB"]
    for k in legs:
        lines.append(f"  {names[k]} per call {_fmt_stat(rec[k]['wall'])} ms  peak allocated "
                     f"{statistics.median(rec[k]['peak']) / 2**20:8.1f} MiB  tail groups batched {groups[k][0]}, per-frame {groups[k][1]}")
    m, c = last["N"].float(), last["C"].float()
    diff = int((last["N"].view(torch.int16) != last["C"].view(torch.int16)).sum())
    lines.append(f"  N against C: {diff} of {m.numel()} bf16 elements differ, largest difference {float((m - c).abs().max()):.3g} "
                 f"(normalised values; one bf16 step near 2 is 0.0156)")
    store.close()
    return lines


class Geom(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bitdepth", C.c_int), ("chroma", C.c_int),
                ("frame_data_type", C.c_int), ("elems", C.c_size_t)]


class RawStore:
    """A latent store and the unchanged formatted render through the C ABI of one libccmi.so."""

    def __init__(self, path, streams, rects, dtype):
        P, I, Z = C.c_void_p, C.c_int, C.c_size_t
        self.L = L = C.CDLL(str(path))
        L.ccmi_last_error.restype = C.c_char_p
        L.ccmi_latents_plan.argtypes = [P, P, I, I, P, P, P]
        L.ccmi_latents_decode.argtypes = [P, P, I, I, P, Z, P, Z, P, P]
        L.ccmi_latents_free.argtypes = [P]
        L.ccmi_latents_free.restype = None
        L.ccmi_latents_render_fmt_plan.argtypes = [P, P, I, P, I, I, P, P, P, P]
        L.ccmi_latents_render_fmt.argtypes = [P, P, I, P, P, P, P, I, I, P, Z, P]
        self.n = n = len(streams)
        keep, sp, ln = decode._marshal(streams)
        nstore, nws = C.c_size_t(0), C.c_size_t(0)
        self.ok(L.ccmi_latents_plan(sp, ln, n, decode.LATENT_I16, C.byref(nstore), None, C.byref(nws)))
        self.store = torch.empty(max(nstore.value, 256), dtype=torch.uint8, device="cuda")
        ws = torch.empty(max(nws.value, 256), dtype=torch.uint8, device="cuda")
        self.h = C.c_void_p(None)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.ok(L.ccmi_latents_decode(sp, ln, n, decode.LATENT_I16, self.store.data_ptr(), self.store.numel(), ws.data_ptr(),
                                      ws.numel(), self.stream, C.byref(self.h)))
        del ws
        self.rects = (decode.Rect * n)(*[decode.Rect(*r) for r in rects])
        elem = {torch.bfloat16: decode.ELEM_BF16, torch.float32: decode.ELEM_F32, torch.float16: decode.ELEM_F16}[dtype]
        self.fmt = decode.TensorFmt(elem=elem, colour=decode.COLOUR_RGB)
        for c in range(3):
            self.fmt.scale[c], self.fmt.bias[c] = 1.0 / STD[c], -MEAN[c] / STD[c]
        geom, need = (Geom * n)(), C.c_size_t(0)
        self.ok(L.ccmi_latents_render_fmt_plan(self.h, None, n, self.rects, 0, 0, C.byref(self.fmt), geom, None, C.byref(need)))
        self.ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device="cuda")
        self.out = torch.empty(n, 3, SIDE, SIDE, dtype=dtype, device="cuda")
        self.op = (C.c_void_p * n)(*[self.out[i].data_ptr() for i in range(n)])
        self.cap = (C.c_size_t * n)(*[3 * SIDE * SIDE * self.out.element_size()] * n)

    def ok(self, rc):
        if rc:
            sys.exit("decode_resample_ab: %s" % self.L.ccmi_last_error().decode(errors="replace"))

    def render(self):
        self.ok(self.L.ccmi_latents_render_fmt(self.h, None, self.n, self.rects, self.op, self.cap, C.byref(self.fmt), 0, 0,
                                               self.ws.data_ptr(), self.ws.numel(), self.stream))

    def close(self):
        self.L.ccmi_latents_free(self.h)


def mode_regress(a, streams):
    if not a.parent or not Path(a.parent).exists():
        sys.exit("decode_resample_ab: --mode regress needs --parent, a libccmi.so built from the parent commit")
    n = len(streams)
    rng = np.random.default_rng(17)
    rects = [(2 * int(rng.integers(0, (W - SIDE) // 2 + 1)), 2 * int(rng.integers(0, (H - SIDE) // 2 + 1)), SIDE, SIDE)
             for _ in range(n)]
    import ccmi
    dtype = getattr(torch, a.dtype)
    libs = {"parent": RawStore(a.parent, streams, rects, dtype), "new": RawStore(ccmi.LIB_PATH, streams, rects, dtype)}
    blocks = 3
    reps = blocks * a.reps
    rec = {k: [] for k in libs}
    for it in range(a.warmup + reps):
        for k, s in libs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.render()
            torch.cuda.synchronize()
            if it >= a.warmup:
                rec[k].append(1e3 * (time.perf_counter() - t0))
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    same = bool((libs["parent"].out.view(bits) == libs["new"].out.view(bits)).all())
    med = {k: [statistics.median(v[b * a.reps:(b + 1) * a.reps]) for b in range(blocks)] for k, v in rec.items()}
    ref, spread = min(med["parent"]), max(med["parent"]) - min(med["parent"])
    new = statistics.median(med["new"])
    lines = ["regression check: the unchanged render_model (no size), parent library against this tree's, one process, alternating",
             f"device: {torch.cuda.get_device_name(0)}; {n} class-E frames, {SIDE}x{SIDE} regions at random even origins, RGB, "
             f"ImageNet mean / std, {a.dtype}, NCHW; {blocks} blocks of {a.reps} alternating repetitions after {a.warmup} warm-up rounds; "
             "wall ms per call",
             "  parent block medians " + ", ".join(f"{v:.3f}" for v in med["parent"]) + f"  (reference {ref:.3f}, spread {spread:.3f})",
             "  new block medians    " + ", ".join(f"{v:.3f}" for v in med["new"]) +
             f"  (median {new:.3f}; limit {ref + spread:.3f})  {'ok' if new <= ref + spread else 'OUTSIDE the allowance'}",
             f"  all repetitions: parent {_fmt_stat(rec['parent'])}  new {_fmt_stat(rec['new'])}",
             f"  outputs equal in every element: {same}"]
    for s in libs.values():
        s.close()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=("resample", "regress"), default="resample")
    ap.add_argument("--parent", default="", help="--mode regress: a libccmi.so built from the parent commit")
    ap.add_argument("--dtype", choices=("bfloat16", "float32", "float16"), default="bfloat16",
                    help="--mode regress: the element type of the rendered tensor")
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "decode_resample_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_resample_ab: no HIP device (this is a GPU measurement)")
    if a.reps < 7:
        sys.exit("decode_resample_ab: at least 7 repetitions")
    files = sorted((ROOT / "tests/golden/cool").glob("E-*.cool"))
    streams = [f.read_bytes() for _ in range(a.copies) for f in files]
    lines = (mode_resample if a.mode == "resample" else mode_regress)(a, streams)
    text = "\n".join(lines + [""])
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
