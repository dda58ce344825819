"""A/B of the colour stage of the output kernels (LatentStore.render_model(colour_ops=...): per-frame
ColorJitter-style brightness / contrast / saturation / hue ops, each frame in its own order, applied
in the decoder's output stage between the resample and the normalisation) against the path it
replaces, on one GPU, in one process, legs alternating, on the bench's `bitexact_decode` set (the 15
committed class-E 1280x720 streams x 64 = 960 frames) held in an int16 LatentStore.  Regions:
RandomResizedCrop (tools/decode_resample_ab.py's, seeded) resampled to 224 x 224; ops:
decode.colour_jitter(n, 0.4, 0.4, 0.4, 0.1) (seeded); RGB, ImageNet mean / std, bfloat16.
  N   store.render_model(roi=..., size=(224, 224), colour_ops=..., mean=..., std=..., dtype=bfloat16)
  C   the composed path: store.render_model(roi=..., size=(224, 224), dtype=float32) (scale 1, bias
      0: one call, one tail group), then the same ops as torch operations, vectorised over the
      frames as far as the per-frame orders allow: for each of the 4 op positions and each of the 4
      kinds, the frames whose op at that position is of that kind are gathered, put through the op
      with their factors as a [m, 1, 1, 1] tensor (the contrast mean: one .mean() over the subset's
      frames) and scattered back; then * scale + bias and the cast to bfloat16.
Warm-up rounds of both legs, then `--reps` (>= 7) alternating wall-clock repetitions, each ended by a
device synchronise.  Reported per leg: median and range of the time per call and of the tail's
device time (decode.last_timing()), the peak of torch's allocated bytes above what was allocated
before the leg (store and workspaces are the caller's, allocated before) and the tail groups.  A
third leg, P, is N without colour_ops (the unchanged call): what the colour stage adds.  The results
are compared: N follows the contract's float32 order and its fixed-point mean, torch its own, so they
differ in rounding (counted, not asserted).

--mode regress: the unchanged call, render_model(roi=..., size=(224, 224)) without ops, through the C
ABI (ccmi_latents_render_rs) of two libraries in one process, alternating, under the rule of
profiles/decode_split_ab.txt: the new library's median of block medians must lie inside the parent's
own spread of block medians.

Run each mode twice; the report is appended to --out."""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "cool-chic_amd"))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import decode_resample_ab as rs_ab  # noqa: E402
from ccmi import decode  # noqa: E402

OUT = rs_ab.OUT
MEAN, STD = rs_ab.MEAN, rs_ab.STD
W, H = rs_ab.W, rs_ab.H
GREY = (0.2989, 0.587, 0.114)


def torch_jitter(x, ops):
    """The ops of every frame of x [n, 3, h, w] (float32, in place where it can), as torch operations."""
    n = x.shape[0]
    dev = x.device
    gw = torch.tensor(GREY, device=dev).view(1, 3, 1, 1)
    depth = max(len(o) for o in ops)
    for k in range(depth):
        for kind in ("brightness", "saturation", "contrast", "matrix"):
            js = [j for j in range(n) if len(ops[j]) > k and ops[j][k][0] == kind]
            if not js:
                continue
            idx = torch.tensor(js, device=dev)
            sub = x.index_select(0, idx)
            if kind == "matrix":
                m = torch.from_numpy(np.stack([np.asarray(ops[j][k][1], np.float32).reshape(3, 4) for j in js])).to(dev)
                sub = (torch.einsum("nck,nkhw->nchw", m[:, :, :3], sub) + m[:, :, 3].view(-1, 3, 1, 1)).clamp_(0, 1)
            else:
                f = torch.tensor([float(ops[j][k][1]) for j in js], device=dev).view(-1, 1, 1, 1)
                if kind == "brightness":
                    sub = (sub * f).clamp_(0, 1)
                else:
                    g = (sub * gw).sum(1, keepdim=True)
                    if kind == "contrast":
                        g = g.mean(dim=(2, 3), keepdim=True)
                    sub = (sub * f + g * (1 - f)).clamp_(0, 1)
            x.index_copy_(0, idx, sub)
    return x


def mode_colour(a, streams):
    n = len(streams)
    rng = np.random.default_rng(17)
    rects = rs_ab.rrc_rects(n, rng)
    ops = decode.colour_jitter(n, 0.4, 0.4, 0.4, 0.1, generator=torch.Generator().manual_seed(29))
    store = decode.LatentStore(streams, dtype=torch.int16)
    scale = torch.tensor([float(np.float32(1.0 / s)) for s in STD], device="cuda").view(1, 3, 1, 1)
    bias = torch.tensor([float(np.float32(-m / s)) for m, s in zip(MEAN, STD)], device="cuda").view(1, 3, 1, 1)
    need_p = store.render_model_workspace_bytes(roi=rects, size=OUT)
    need_n = store.render_model_workspace_bytes(roi=rects, size=OUT, colour_ops=ops)
    ws = torch.empty(max(need_n, 256), dtype=torch.uint8, device="cuda")

    def leg_new():
        out = store.render_model(roi=rects, size=OUT, colour_ops=ops, mean=MEAN, std=STD, dtype=torch.bfloat16, workspace=ws)
        return out, decode.last_tail_groups(), decode.last_timing()["ups_syn_out"]

    def leg_plain():
        out = store.render_model(roi=rects, size=OUT, mean=MEAN, std=STD, dtype=torch.bfloat16, workspace=ws)
        return out, decode.last_tail_groups(), decode.last_timing()["ups_syn_out"]

    def leg_composed():
        x = store.render_model(roi=rects, size=OUT, dtype=torch.float32, workspace=ws)
        groups, tail = decode.last_tail_groups(), decode.last_timing()["ups_syn_out"]
        x = torch_jitter(x, ops)
        return (x * scale + bias).to(torch.bfloat16), groups, tail

    legs = {"N": leg_new, "C": leg_composed, "P": leg_plain}
    rec = {k: {"wall": [], "tail": [], "peak": []} for k in legs}
    last, groups = {}, {}
    for it in range(a.warmup + a.reps):
        for k, fn in legs.items():
            last[k] = None
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            last[k], groups[k], tail = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if it >= a.warmup:
                rec[k]["wall"].append(1e3 * dt)
                rec[k]["tail"].append(tail)
                rec[k]["peak"].append(torch.cuda.max_memory_allocated() - base)
    names = {"N": "N  render_model(size=, colour_ops=)           ", "C": "C  render_model(size=, float32) + torch ops   ",
             "P": "P  render_model(size=), no ops (unchanged)    "}
    orders = len({tuple(op for op, _ in o) for o in ops})
    lines = ["colour stage A/B: LatentStore.render_model(size=..., colour_ops=...) against render_model(size=..., float32) + the "
             "same ops as torch operations, alternating",
             f"device: {torch.cuda.get_device_name(0)}; one process; {n} class-E frames of {W}x{H}; RandomResizedCrop regions -> "
             f"{OUT[0]}x{OUT[1]}; colour_jitter(0.4, 0.4, 0.4, 0.1): 4 ops per frame, {orders} distinct orders; bf16 RGB normalised; "
             f"median [min .. max] of {a.reps} repetitions after {a.warmup} warm-up rounds; workspace (caller-owned, not in the "
             f"peaks): {need_n / 2**20:.1f} MiB with ops, {need_p / 2**20:.1f} MiB without ({need_n - need_p} bytes more)"]
    for k in legs:
        lines.append(f"  {names[k]} per call {rs_ab._fmt_stat(rec[k]['wall'])} ms  tail {rs_ab._fmt_stat(rec[k]['tail'])} ms  "
                     f"peak allocated {statistics.median(rec[k]['peak']) / 2**20:8.1f} MiB  tail groups batched {groups[k][0]}, "
                     f"per-frame {groups[k][1]}")
    mm, c = last["N"].float(), last["C"].float()
    diff = int((last["N"].view(torch.int16) != last["C"].view(torch.int16)).sum())
    lines.append(f"  N against C: {diff} of {mm.numel()} bf16 elements differ ({100.0 * diff / mm.numel():.3f} %), largest difference "
                 f"{float((mm - c).abs().max()):.3g} (normalised values; one bf16 step near 2 is 0.0156)")
    store.close()
    return lines


class RawStoreRs(rs_ab.RawStore):
    """rs_ab.RawStore with the resampling render: regions of any size to OUT through ccmi_latents_render_rs."""

    def __init__(self, path, streams, rects, dtype):
        super().__init__(path, streams, rects, dtype)
        P, I, Z = C.c_void_p, C.c_int, C.c_size_t
        L, n = self.L, self.n
        L.ccmi_latents_render_rs_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P]
        L.ccmi_latents_render_rs.argtypes = [P, P, I, P, P, P, P, P, I, I, P, Z, P]
        self.rs = decode.Resample(out_w=OUT[1], out_h=OUT[0], filter=decode.FILTER_TRIANGLE)
        geom, need = (rs_ab.Geom * n)(), C.c_size_t(0)
        self.ok(L.ccmi_latents_render_rs_plan(self.h, None, n, self.rects, 0, 0, C.byref(self.fmt), C.byref(self.rs), geom, None,
                                              C.byref(need)))
        self.ws = None
        self.ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device="cuda")
        self.out = None
        self.out = torch.empty(n, 3, *OUT, dtype=dtype, device="cuda")
        self.op = (C.c_void_p * n)(*[self.out[i].data_ptr() for i in range(n)])
        self.cap = (C.c_size_t * n)(*[3 * OUT[0] * OUT[1] * self.out.element_size()] * n)

    def render(self):
        self.ok(self.L.ccmi_latents_render_rs(self.h, None, self.n, self.rects, self.op, self.cap, C.byref(self.fmt),
                                              C.byref(self.rs), 0, 0, self.ws.data_ptr(), self.ws.numel(), self.stream))


def mode_regress(a, streams):
    if not a.parent or not Path(a.parent).exists():
        sys.exit("decode_colour_ab: --mode regress needs --parent, a libccmi.so built from the parent commit")
    import ccmi
    n = len(streams)
    rects = rs_ab.rrc_rects(n, np.random.default_rng(17))
    dtype = torch.bfloat16
    libs = {"parent": RawStoreRs(a.parent, streams, rects, dtype), "new": RawStoreRs(ccmi.LIB_PATH, streams, rects, dtype)}
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
    same = bool((libs["parent"].out.view(torch.int16) == libs["new"].out.view(torch.int16)).all())
    med = {k: [statistics.median(v[b * a.reps:(b + 1) * a.reps]) for b in range(blocks)] for k, v in rec.items()}
    ref, spread = min(med["parent"]), max(med["parent"]) - min(med["parent"])
    new = statistics.median(med["new"])
    lines = ["regression check: the unchanged render_model(size=) (no ops), parent library against this tree's, one process, "
             "alternating",
             f"device: {torch.cuda.get_device_name(0)}; {n} class-E frames, RandomResizedCrop regions -> {OUT[0]}x{OUT[1]}, RGB, "
             f"ImageNet mean / std, bfloat16, NCHW; {blocks} blocks of {a.reps} alternating repetitions after {a.warmup} warm-up "
             "rounds; wall ms per call",
             "  parent block medians " + ", ".join(f"{v:.3f}" for v in med["parent"]) + f"  (reference {ref:.3f}, spread {spread:.3f})",
             "  new block medians    " + ", ".join(f"{v:.3f}" for v in med["new"]) +
             f"  (median {new:.3f}; limit {ref + spread:.3f})  {'ok' if new <= ref + spread else 'OUTSIDE the allowance'}",
             f"  all repetitions: parent {rs_ab._fmt_stat(rec['parent'])}  new {rs_ab._fmt_stat(rec['new'])}",
             f"  outputs equal in every element: {same}"]
    for s in libs.values():
        s.close()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=("colour", "regress"), default="colour")
    ap.add_argument("--parent", default="", help="--mode regress: a libccmi.so built from the parent commit")
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "decode_colour_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_colour_ab: no HIP device (this is a GPU measurement)")
    if a.reps < 7:
        sys.exit("decode_colour_ab: at least 7 repetitions")
    files = sorted((ROOT / "tests/golden/cool").glob("E-*.cool"))
    streams = [f.read_bytes() for _ in range(a.copies) for f in files]
    lines = (mode_colour if a.mode == "colour" else mode_regress)(a, streams)
    text = "\n".join(lines + [""])
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
