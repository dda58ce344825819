"""A/B of the mix stage of the decoder's output stage (LatentStore.render_model(erase=..., erase_seed=...,
mix=...): RandomErasing, MixUp and CutMix after the normalisation and before the rounding to bfloat16)
against the path it replaces, on one GPU, in one process, legs alternating, in the form of
tools/decode_tone_ab.py and on its workload: the bench's `bitexact_decode` set (the 15 committed class-E
1280x720 streams x 64 = 960 frames) held in an int16 LatentStore, RandomResizedCrop windows x
decode.rand_augment(n, num_ops=2, magnitude=9) warped to 224 x 224, RGB, ImageNet mean / std, bfloat16
(the README's RandAugment row), plus decode.random_erasing(n, p=0.25, value="pixel") and
decode.mixup_cutmix(n, 0.8, 1.0, pairing="roll", per_frame=True) (all seeded; a decision per frame, so one
call holds blends and boxes).
  N   store.render_model(affine=..., size=(224, 224), tone_ops=..., erase=..., erase_seed=..., mix=..., bf16)
  P   the same call without the stage (the call of the RandAugment row): what the stage adds.
  C   the composed path: P, then the same steps as torch operations on the finished bfloat16 tensor: per
      frame x[j, :, y:y+h, x:x+w].normal_() (torch's global generator), then rolled = batch.roll(1, 0),
      x.mul_(lam).add_(rolled * (1 - lam)) with lam per frame (1 where a frame does not blend) and, per
      CutMix frame, the box copied from the rolled batch.
Warm-up rounds of all legs, then `--reps` (>= 7) alternating wall-clock repetitions, each ended by a device
synchronise.  Reported per leg: median and range of the time per call and of the tail's device time
(decode.last_timing(); the mix launch ends the tail), the peak of torch's allocated bytes above what was
allocated before the leg (store and workspaces are the caller's, allocated before), the tail groups, and
the workspace growth, and the host's share: the Python marshalling of erase= / mix= alone and the header-only
plan call with and without the stage (wall clock, no GPU work).  After the timed rounds N and C run once more with CONSTANT rectangles (value 0) for
an element-for-element comparison: the share of bf16 elements that differ and by how many bf16 steps (C
rounds to bfloat16 before it mixes, N after: counted, not asserted).

--mode regress: the unchanged call, tools/decode_filter_ab.py's regression check (render_model(size=,
colour_ops=) through ccmi_latents_render_col of the parent's library and this tree's, alternating; the new
median of block medians inside the parent's own spread, outputs equal in every element).
--mode regress-tone: the same check through ccmi_latents_render_tone(_plan) with tone and filter NULL, the
entry points that are now the mix == NULL case of the _mix ones.

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

import torch  # noqa: E402

import decode_filter_ab as flt_ab  # noqa: E402
import decode_resample_ab as rs_ab  # noqa: E402
import decode_tone_ab as tone_ab  # noqa: E402
from ccmi import decode  # noqa: E402

OUT = rs_ab.OUT
MEAN, STD = rs_ab.MEAN, rs_ab.STD
W, H = rs_ab.W, rs_ab.H


def workload(n):
    mats, tones = tone_ab.workload(n)
    g = torch.Generator().manual_seed(43)
    erase, seeds = decode.random_erasing(n, OUT, p=0.25, value="pixel", generator=g)
    mix, lab = decode.mixup_cutmix(n, OUT, mixup_alpha=0.8, cutmix_alpha=1.0, pairing="roll", per_frame=True, generator=g)
    return mats, tones, erase, seeds, mix


def torch_mix(x, erase, mix, constant):
    """the erase lists and the mix of every frame of x [n, 3, h, w], in place, as torch operations"""
    for j, e in enumerate(erase):
        for rx, ry, rw, rh, v, sigma in e or ():
            if constant:
                x[j, :, ry: ry + rh, rx: rx + rw] = v
            else:
                x[j, :, ry: ry + rh, rx: rx + rw].normal_(v, sigma)
    if all(m is None for m in mix):
        return x
    rolled = x.roll(1, 0)  # frame j's partner is frame j - 1
    lam = torch.tensor([1.0 if m is None or hasattr(m[1], "__len__") else m[1] for m in mix], device=x.device, dtype=x.dtype)
    lam = lam.view(-1, 1, 1, 1)
    x.mul_(lam).add_(rolled * (1.0 - lam))
    for j, m in enumerate(mix):
        if m is not None and hasattr(m[1], "__len__"):
            bx, by, bw, bh = m[1]
            x[j, :, by: by + bh, bx: bx + bw] = rolled[j, :, by: by + bh, bx: bx + bw]
    return x


def mode_mix(a, streams):
    n = len(streams)
    mats, tones, erase, seeds, mix = workload(n)
    const = [None if e is None else [r[:4] + (0.0, 0.0) for r in e] for e in erase]
    store = decode.LatentStore(streams, dtype=torch.int16)
    geo = dict(affine=mats, size=OUT, fill=0.0, tone_ops=tones)
    need_p = store.render_model_workspace_bytes(**geo)
    need_n = store.render_model_workspace_bytes(erase=erase, mix=mix, **geo)
    ws = torch.empty(max(need_n, 256), dtype=torch.uint8, device="cuda")
    fmt = dict(mean=MEAN, std=STD, dtype=torch.bfloat16)

    def leg_new(er=erase):
        out = store.render_model(erase=er, erase_seed=seeds, mix=mix, workspace=ws, **geo, **fmt)
        return out, decode.last_tail_groups(), decode.last_timing()["ups_syn_out"]

    def leg_plain():
        out = store.render_model(workspace=ws, **geo, **fmt)
        return out, decode.last_tail_groups(), decode.last_timing()["ups_syn_out"]

    def leg_composed(er=erase, constant=False):
        x, groups, tail = leg_plain()
        return torch_mix(x, er, mix, constant), groups, tail

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
    names = {"N": "N  render_model(affine=, size=, tone_ops=, erase=, mix=)       ",
             "C": "C  render_model(affine=, size=, tone_ops=) + torch ops         ",
             "P": "P  render_model(affine=, size=, tone_ops=), no mix (unchanged) "}
    erased = sum(e is not None for e in erase)
    mixed = sum(m is not None for m in mix)
    boxes = sum(m is not None and hasattr(m[1], "__len__") for m in mix)
    kind = f"{mixed - boxes} blends and {boxes} boxes"
    staged = len({j for j, (e, m) in enumerate(zip(erase, mix)) if e is not None or m is not None}
                 | {m[0] for m in mix if m is not None})
    lines = ["mix stage A/B: LatentStore.render_model(affine=..., size=..., tone_ops=..., erase=..., mix=...) against the same call "
             "without the stage + the steps as torch operations on the bf16 tensor, alternating",
             f"device: {torch.cuda.get_device_name(0)}; one process; {n} class-E frames of {W}x{H}; RandomResizedCrop windows x "
             f"rand_augment(num_ops=2, magnitude=9) -> {OUT[0]}x{OUT[1]}; random_erasing(p=0.25, 'pixel'): {erased} frames; "
             f"mixup_cutmix(0.8, 1.0, roll, per frame): {mixed} frames, {kind}; {staged} frames are mix-staged; bf16 RGB normalised; median "
             f"[min .. max] of {a.reps} repetitions after {a.warmup} warm-up rounds; workspace (caller-owned, not in the peaks): "
             f"{need_n / 2**20:.1f} MiB with the stage, {need_p / 2**20:.1f} MiB without ({need_n - need_p} bytes more)"]
    for k in legs:
        lines.append(f"  {names[k]} per call {rs_ab._fmt_stat(rec[k]['wall'])} ms  tail {rs_ab._fmt_stat(rec[k]['tail'])} ms  "
                     f"peak allocated {statistics.median(rec[k]['peak']) / 2**20:8.1f} MiB  tail groups batched {groups[k][0]}, "
                     f"per-frame {groups[k][1]}")
    d = statistics.median(rec["N"]["wall"]) - statistics.median(rec["P"]["wall"])
    lines.append(f"  the stage costs {d:.2f} ms per call (N - P, medians); the composed path "
                 f"{statistics.median(rec['C']['wall']) - statistics.median(rec['P']['wall']):.2f} ms")
    # where the host's share of N - P goes: the Python marshalling alone, and the header-only plan call (which
    # marshals, validates and lays out, and which a render repeats before it fills and uploads the tables)
    def host_ms(fn):
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            ts.append(1e3 * (time.perf_counter() - t0))
        return ts
    marshal = host_ms(lambda: decode._mix(erase, seeds, mix, n))
    plan_n = host_ms(lambda: store.render_model_workspace_bytes(erase=erase, erase_seed=seeds, mix=mix, **geo))
    plan_p = host_ms(lambda: store.render_model_workspace_bytes(**geo))
    lines.append(f"  host side, no GPU work: decode._mix() marshalling {rs_ab._fmt_stat(marshal)} ms; the plan call with the stage "
                 f"{rs_ab._fmt_stat(plan_n)} ms, without {rs_ab._fmt_stat(plan_p)} ms")
    cn, cc = leg_new(const)[0], leg_composed(const, True)[0]
    torch.cuda.synchronize()
    steps = flt_ab.bf16_steps(cn, cc)
    diff, total = int((steps != 0).sum()), steps.numel()
    hist = ", ".join(f"{k} step{'s' if k > 1 else ''}: {int((steps == k).sum())}" for k in (1, 2, 3))
    lines.append(f"  constant rectangles, N against C: {diff} of {total} bf16 elements differ ({100.0 * diff / total:.3f} %); {hist}; "
                 f"more than 3: {int((steps > 3).sum())}; largest {int(steps.max())} steps")
    store.close()
    return lines


class RawStoreTone(flt_ab.RawStoreCol):
    """flt_ab.RawStoreCol through the _tone entry points (tone NULL, filter NULL: the same call)."""

    def __init__(self, path, streams, rects, dtype, ops):
        super().__init__(path, streams, rects, dtype, ops)
        P, I, Z = C.c_void_p, C.c_int, C.c_size_t
        L, n = self.L, self.n
        L.ccmi_latents_render_tone_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P, P, P]
        L.ccmi_latents_render_tone.argtypes = [P, P, I, P, P, P, P, P, P, P, P, P, I, I, P, Z, P]
        geom, need = (rs_ab.Geom * n)(), C.c_size_t(0)
        self.ok(L.ccmi_latents_render_tone_plan(self.h, None, n, self.rects, 0, 0, C.byref(self.fmt), C.byref(self.rs), None,
                                                C.byref(self.col), None, None, geom, None, None, C.byref(need)))
        assert need.value == self.need  # the _col plan's

    def render(self):
        self.ok(self.L.ccmi_latents_render_tone(self.h, None, self.n, self.rects, self.op, self.cap, C.byref(self.fmt),
                                                C.byref(self.rs), None, C.byref(self.col), None, None, 0, 0, self.ws.data_ptr(),
                                                self.ws.numel(), self.stream))


def mode_regress_tone(a, streams):
    """flt_ab.mode_regress with the call made through ccmi_latents_render_tone"""
    col = flt_ab.RawStoreCol
    flt_ab.RawStoreCol = RawStoreTone
    try:
        lines = flt_ab.mode_regress(a, streams)
    finally:
        flt_ab.RawStoreCol = col
    lines[0] = lines[0].replace("through ccmi_latents_render_col", "through ccmi_latents_render_tone (tone NULL, filter NULL)")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=("mix", "regress", "regress-tone"), default="mix")
    ap.add_argument("--parent", default="", help="--mode regress: a libccmi.so built from the parent commit")
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "decode_mix_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_mix_ab: no HIP device (this is a GPU measurement)")
    if a.reps < 7:
        sys.exit("decode_mix_ab: at least 7 repetitions")
    files = sorted((ROOT / "tests/golden/cool").glob("E-*.cool"))
    streams = [f.read_bytes() for _ in range(a.copies) for f in files]
    lines = {"mix": mode_mix, "regress": flt_ab.mode_regress, "regress-tone": mode_regress_tone}[a.mode](a, streams)
    text = "\n".join(lines + [""])
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
