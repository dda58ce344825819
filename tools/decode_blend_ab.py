"""A/B of the blend stage of the decoder's output stage (LatentStore.render_model(blend=..., silent=...): AugMix's
weighted sum of differently augmented renders of one frame, before the normalisation and the one rounding to
bfloat16) against the paths it replaces, on one GPU, in one process, legs alternating, in the form of
tools/decode_mix_ab.py: the bench's `bitexact_decode` set (the 15 committed class-E 1280x720 streams x 64 =
960 frames) held in an int16 LatentStore, RandomResizedCrop windows as the base matrices,
decode.aug_mix(n, (224, 224), severity=3, mixture_width=3) (seeded): 3840 rendered frames for 960 outputs,
224 x 224, RGB, ImageNet mean / std, bfloat16.
  N   store.render_model(index=repeat, affine=..., size=(224, 224), tone_ops=..., blend=..., silent=..., bf16)
  A   the same 3840-frame call without blend, every frame emitting (bf16): what rendering the chains costs.
  B   the composed path: that call in float32 (mean 0, std 1), then the weighted sum, the normalisation and
      the cast as torch operations.
Warm-up rounds of all legs, then `--reps` (>= 7) alternating wall-clock repetitions, each ended by a device
synchronise.  Reported per leg: median and range of the time per call and of the tail's device time
(decode.last_timing(); the blend launch ends the tail), the peak of torch's allocated bytes above what was
allocated before the leg (store and workspaces are the caller's, allocated before), the tail groups and the
workspaces; then the share of bf16 elements of N that differ from B and by how many bf16 steps (counted, not
asserted: B sums with torch's fused kernels).

--mode regress: the unchanged call, ccmi_latents_render_mix of tools/decode_mix_ab.py's workload (the README's
mix row) through the parent's library and this tree's, alternating: the new median of block medians inside
the parent's own spread, outputs equal in every element.

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

import decode_colour_ab as col_ab  # noqa: E402
import decode_filter_ab as flt_ab  # noqa: E402
import decode_mix_ab as mix_ab  # noqa: E402
import decode_resample_ab as rs_ab  # noqa: E402
from ccmi import decode  # noqa: E402

OUT = rs_ab.OUT
MEAN, STD = rs_ab.MEAN, rs_ab.STD
W, H = rs_ab.W, rs_ab.H
WIDTH = 3


def workload(n):
    rects = rs_ab.rrc_rects(n, np.random.default_rng(17))
    base = np.array([[[w / OUT[1], 0.0, x], [0.0, h / OUT[0], y]] for x, y, w, h in rects])
    return decode.aug_mix(n, OUT, severity=3, mixture_width=WIDTH, generator=torch.Generator().manual_seed(47), base=base)


def mode_blend(a, streams):
    n = len(streams)
    am = workload(n)
    m = len(am["repeat"])
    store = decode.LatentStore(streams, dtype=torch.int16)
    geo = dict(index=[int(r) for r in am["repeat"]], affine=am["matrices"], size=OUT, fill=0.0, tone_ops=am["tone_ops"])
    need_a = store.render_model_workspace_bytes(**geo)
    need_n = store.render_model_workspace_bytes(blend=am["blend"], silent=am["silent"], **geo)
    ws = torch.empty(max(need_n, need_a, 256), dtype=torch.uint8, device="cuda")
    fmt = dict(mean=MEAN, std=STD, dtype=torch.bfloat16)
    scale = torch.tensor([float(np.float32(1.0 / s)) for s in STD], device="cuda").view(1, 3, 1, 1)
    bias = torch.tensor([float(np.float32(-mu / s)) for mu, s in zip(MEAN, STD)], device="cuda").view(1, 3, 1, 1)
    wts = torch.tensor([[w for _, w in am["blend"][j * (1 + WIDTH)]] for j in range(n)], dtype=torch.float32, device="cuda")

    def leg_new():
        out = store.render_model(blend=am["blend"], silent=am["silent"], workspace=ws, **geo, **fmt)
        return out, decode.last_tail_groups(), decode.last_timing()["ups_syn_out"]

    def leg_all():
        out = store.render_model(workspace=ws, **geo, **fmt)
        return out, decode.last_tail_groups(), decode.last_timing()["ups_syn_out"]

    def leg_composed():
        x = store.render_model(workspace=ws, dtype=torch.float32, **geo)
        groups, tail = decode.last_tail_groups(), decode.last_timing()["ups_syn_out"]
        z = (x.view(n, 1 + WIDTH, 3, *OUT) * wts.view(n, 1 + WIDTH, 1, 1, 1)).sum(dim=1)
        return (z * scale + bias).to(torch.bfloat16), groups, tail

    legs = {"N": leg_new, "B": leg_composed, "A": leg_all}
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
    names = {"N": "N  render_model(affine=, tone_ops=, blend=, silent=): 960 outputs      ",
             "B": "B  the 3840 frames in float32 + torch sum, normalisation, cast         ",
             "A": "A  the 3840 frames without blend, all emitting (bf16)                  "}
    lines = ["blend stage A/B: LatentStore.render_model(index=repeat, affine=..., size=..., tone_ops=..., blend=..., silent=...) against "
             "the same frames without blend, and against their float32 render + the weighted sum, normalisation and cast as torch "
             "operations, alternating",
             f"device: {torch.cuda.get_device_name(0)}; one process; {n} class-E frames of {W}x{H}; RandomResizedCrop windows x "
             f"aug_mix(severity=3, mixture_width={WIDTH}) -> {m} rendered frames of {OUT[0]}x{OUT[1]}, {n} outputs; bf16 RGB normalised; "
             f"median [min .. max] of {a.reps} repetitions after {a.warmup} warm-up rounds; workspace (caller-owned, not in the peaks): "
             f"{need_n / 2**20:.1f} MiB with the stage, {need_a / 2**20:.1f} MiB for the {m} frames without ({need_n - need_a} bytes more)"]
    for k in legs:
        lines.append(f"  {names[k]} per call {rs_ab._fmt_stat(rec[k]['wall'])} ms  tail {rs_ab._fmt_stat(rec[k]['tail'])} ms  "
                     f"peak allocated {statistics.median(rec[k]['peak']) / 2**20:8.1f} MiB  tail groups batched {groups[k][0]}, "
                     f"per-frame {groups[k][1]}")
    steps = flt_ab.bf16_steps(last["N"], last["B"])
    diff, total = int((steps != 0).sum()), steps.numel()
    hist = ", ".join(f"{k} step{'s' if k > 1 else ''}: {int((steps == k).sum())}" for k in (1, 2, 3))
    lines.append(f"  N against B: {diff} of {total} bf16 elements differ ({100.0 * diff / total:.3f} %); {hist}; more than 3: "
                 f"{int((steps > 3).sum())}; largest {int(steps.max())} steps")
    # the traffic model of the launch: 12 K bytes read and 3 sizeof(bf16) written per output pixel, K = 1 + width
    px = n * OUT[0] * OUT[1]
    lines.append(f"  traffic model of dec_blend_batch for this call: {px * (12 * (1 + WIDTH) + 6) / 2**20:.1f} MiB "
                 f"({12 * (1 + WIDTH)} bytes read and 6 written per output pixel)")
    store.close()
    return lines


class RawStoreMix(col_ab.RawStoreRs):
    """col_ab.RawStoreRs with the mix row's call: warp, tone ops, erase and mix through ccmi_latents_render_mix."""

    def __init__(self, path, streams, rects, dtype, work):
        super().__init__(path, streams, rects, dtype)
        P, I, Z = C.c_void_p, C.c_int, C.c_size_t
        L, n = self.L, self.n
        L.ccmi_latents_render_mix_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P, P, P, P]
        L.ccmi_latents_render_mix.argtypes = [P, P, I, P, P, P, P, P, P, P, P, P, P, I, I, P, Z, P]
        mats, tones, erase, seeds, mix = work
        self.warp, self.keep_w = decode._warp(mats, n, OUT, None, "fill", 0.0, decode._interp("bilinear", False), None)
        self.tone, self.keep_t = decode._tone(tones, n)
        self.mx, self.keep_m = decode._mix(erase, seeds, mix, n)
        geom, need = (rs_ab.Geom * n)(), C.c_size_t(0)
        self.ok(L.ccmi_latents_render_mix_plan(self.h, None, n, None, 0, 0, C.byref(self.fmt), None, C.byref(self.warp), None,
                                               C.byref(self.tone), None, C.byref(self.mx), geom, None, None, C.byref(need)))
        self.need = need.value
        self.ws = None
        self.ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device="cuda")

    def render(self):
        self.ok(self.L.ccmi_latents_render_mix(self.h, None, self.n, None, self.op, self.cap, C.byref(self.fmt), None,
                                               C.byref(self.warp), None, C.byref(self.tone), None, C.byref(self.mx), 0, 0,
                                               self.ws.data_ptr(), self.ws.numel(), self.stream))


def mode_regress(a, streams):
    if not a.parent or not Path(a.parent).exists():
        sys.exit("decode_blend_ab: --mode regress needs --parent, a libccmi.so built from the parent commit")
    import ccmi
    n = len(streams)
    work = mix_ab.workload(n)
    rects = rs_ab.rrc_rects(n, np.random.default_rng(17))  # the base class's plan; the mix row's call takes none
    dtype = torch.bfloat16
    libs = {"parent": RawStoreMix(a.parent, streams, rects, dtype, work), "new": RawStoreMix(ccmi.LIB_PATH, streams, rects, dtype, work)}
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
    lines = ["regression check: the unchanged call of the mix row, render_model(affine=, tone_ops=, erase=, mix=) through "
             "ccmi_latents_render_mix, parent library against this tree's, one process, alternating",
             f"device: {torch.cuda.get_device_name(0)}; {n} class-E frames, RandomResizedCrop windows x rand_augment -> {OUT[0]}x{OUT[1]}, "
             f"random_erasing(p=0.25, 'pixel'), mixup_cutmix(0.8, 1.0), RGB, ImageNet mean / std, bfloat16, NCHW; {blocks} blocks of "
             f"{a.reps} alternating repetitions after {a.warmup} warm-up rounds; wall ms per call; workspace parent "
             f"{libs['parent'].need} bytes, new {libs['new'].need} bytes",
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
    ap.add_argument("--mode", choices=("blend", "regress"), default="blend")
    ap.add_argument("--parent", default="", help="--mode regress: a libccmi.so built from the parent commit")
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "decode_blend_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_blend_ab: no HIP device (this is a GPU measurement)")
    if a.reps < 7:
        sys.exit("decode_blend_ab: at least 7 repetitions")
    files = sorted((ROOT / "tests/golden/cool").glob("E-*.cool"))
    streams = [f.read_bytes() for _ in range(a.copies) for f in files]
    lines = (mode_blend if a.mode == "blend" else mode_regress)(a, streams)
    text = "\n".join(lines + [""])
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
