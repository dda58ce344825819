"""Everything the decoder's header-only entry points answer, one JSON line per call, for an
A/B of two builds of libccmi.so (the planner is host arithmetic: no GPU needed):

    CCMI_LIB=<parent>/libccmi.so python tools/decode_plan_ab.py > a.jsonl
    python tools/decode_plan_ab.py > b.jsonl && cmp a.jsonl b.jsonl

Calls ccmi_decode_output_size, ccmi_decode_batch_workspace_bytes, ccmi_decode_batch_plan,
ccmi_decode_batch_dev_plan and ccmi_decode_batch_dev_roi_plan on every committed stream
(tests/golden/cool, tests/golden/cool_synth): alone and in batches of 7 and 66, for output
bitdepth 0 / 8 / 10 / 16, chroma 0 / 420 / 444, the three sample types and as_yuv 0 / 1; the
region plan over a fixed list of rectangles per frame (whole frame, 1x1 corners, odd origins,
each border touched, one sample outside each border, a few seeded random ones); and every
entry point on every stream truncated at each length from 0 to its header size plus 8.
Each line holds the return code, the error message and every output value."""
import ctypes as C
import json
import os
import random
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
LIB = Path(os.environ.get("CCMI_LIB", ROOT / "cool-chic_amd" / "lib" / "libccmi.so"))
FILES = sorted((ROOT / "tests" / "golden" / "cool").rglob("*.cool")) + \
    sorted((ROOT / "tests" / "golden" / "cool_synth").rglob("*.cool"))
BITDEPTHS, CHROMAS, SAMPLES = (0, 8, 10, 16), (0, 420, 444), (0, 1, 2)
MAX_GRIDS = 8


class Geom(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bitdepth", C.c_int), ("chroma", C.c_int),
                ("frame_data_type", C.c_int), ("elems", C.c_size_t)]


class Rect(C.Structure):
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("w", C.c_int), ("h", C.c_int)]


class RoiInfo(C.Structure):
    _fields_ = [("n_grids", C.c_int), ("arm_rows", C.c_int * MAX_GRIDS), ("windowed", C.c_int)]


lib = C.CDLL(str(LIB))
lib.ccmi_last_error.restype = C.c_char_p
P, I, Z = C.c_void_p, C.c_int, C.c_size_t
for name, args in (("ccmi_decode_output_size", [P, Z, I, I, I, P]),
                   ("ccmi_decode_batch_workspace_bytes", [P, P, I, I, I, I, P]),
                   ("ccmi_decode_batch_plan", [P, P, I, I, I, I, P, P]),
                   ("ccmi_decode_batch_dev_plan", [P, P, I, I, I, I, P, P]),
                   ("ccmi_decode_batch_dev_roi_plan", [P, P, I, P, I, I, I, P, P, P])):
    getattr(lib, name).argtypes = args
    getattr(lib, name).restype = I


def emit(fn, args, rc, out):
    err = lib.ccmi_last_error().decode("utf-8", "replace") if rc else ""
    print(json.dumps({"fn": fn, "args": args, "rc": rc, "err": err, "out": out if rc == 0 else None}))


class Batch:
    def __init__(self, names, data):
        self.names, self.n = names, len(data)
        self.bufs = [C.create_string_buffer(d, len(d)) if d else C.create_string_buffer(1) for d in data]
        self.sp = (C.c_void_p * self.n)(*[C.cast(b, C.c_void_p) for b in self.bufs])
        self.ln = (C.c_size_t * self.n)(*[len(d) for d in data])
        self.lens = [len(d) for d in data]


def geoms(g):
    return [[x.width, x.height, x.bitdepth, x.chroma, x.frame_data_type, x.elems] for x in g]


def call_output_size(b, bd, ch, yuv):
    size = C.c_size_t(0)
    rc = lib.ccmi_decode_output_size(b.sp[0], b.ln[0], bd, ch, yuv, C.byref(size))
    emit("output_size", [b.names[0], b.lens[0], bd, ch, yuv], rc, size.value)


def call_workspace_bytes(b, bd, ch, yuv):
    need = C.c_size_t(0)
    rc = lib.ccmi_decode_batch_workspace_bytes(b.sp, b.ln, b.n, bd, ch, yuv, C.byref(need))
    emit("workspace_bytes", [b.names, b.lens, bd, ch, yuv], rc, need.value)


def call_plan(b, bd, ch, yuv):
    sizes, need = (C.c_size_t * b.n)(), C.c_size_t(0)
    rc = lib.ccmi_decode_batch_plan(b.sp, b.ln, b.n, bd, ch, yuv, sizes, C.byref(need))
    emit("plan", [b.names, b.lens, bd, ch, yuv], rc, [list(sizes), need.value])


def call_dev_plan(b, bd, ch, sample):
    g, need = (Geom * b.n)(), C.c_size_t(0)
    rc = lib.ccmi_decode_batch_dev_plan(b.sp, b.ln, b.n, bd, ch, sample, g, C.byref(need))
    emit("dev_plan", [b.names, b.lens, bd, ch, sample], rc, [geoms(g), need.value])


def call_roi_plan(b, rects, bd, ch, sample):
    g, info, need = (Geom * b.n)(), (RoiInfo * b.n)(), C.c_size_t(0)
    roi = (Rect * b.n)(*[Rect(*r) for r in rects])
    rc = lib.ccmi_decode_batch_dev_roi_plan(b.sp, b.ln, b.n, roi, bd, ch, sample, g, info, C.byref(need))
    infos = [[x.n_grids, list(x.arm_rows), x.windowed] for x in info]
    emit("roi_plan", [b.names, b.lens, rects, bd, ch, sample], rc, [geoms(g), infos, need.value])


def frame_size(d):
    return int.from_bytes(d[4:6], "big"), int.from_bytes(d[2:4], "big")  # w, h (GOP header)


def header_size(d):
    return 9 + int.from_bytes(d[9:11], "big")  # GOP header, then the frame header's own size field


def rects_of(w, h, rng):
    a, b = max(1, w // 3), max(1, h // 3)
    r = [(0, 0, w, h),
         (0, 0, 1, 1), (w - 1, 0, 1, 1), (0, h - 1, 1, 1), (w - 1, h - 1, 1, 1),  # 1x1 at each corner
         (1, 1, max(1, min(33, w - 1)), max(1, min(17, h - 1))), (3, 5, max(1, w - 3), max(1, h - 5)),  # odd origins
         (0, b, a, b), (a, 0, a, b), (w - a, b, a, b), (a, h - b, a, b),  # touching each border
         (-1, b, a, b), (a, -1, a, b), (w - a + 1, b, a, b), (a, h - b + 1, a, b),  # one sample outside each border
         (2, 2, 0, 4), (2, 2, 4, 0)]
    for _ in range(4):
        x, y = rng.randrange(w), rng.randrange(h)
        r.append((x, y, rng.randint(1, w - x), rng.randint(1, h - y)))
    for _ in range(2):  # even origins: what a 420 output takes
        x, y = rng.randrange(w) & ~1, rng.randrange(h) & ~1
        r.append((x, y, rng.randint(1, w - x), rng.randint(1, h - y)))
    return r


def main():
    names = [str(f.relative_to(ROOT / "tests" / "golden")) for f in FILES]
    data = [f.read_bytes() for f in FILES]
    rng = random.Random(20240611)
    rects = [rects_of(*frame_size(d), rng) for d in data]
    n = len(data)
    groups = [[i] for i in range(n)]
    groups += [list(range(i, min(i + 7, n))) for i in range(0, n, 7)]
    groups += [list(range(0, min(66, n))), list(range(max(0, n - 66), n))]
    for grp in groups:
        b = Batch([names[i] for i in grp], [data[i] for i in grp])
        n_rects = len(rects[grp[0]]) if len(grp) == 1 else 8
        for bd in BITDEPTHS:
            for ch in CHROMAS:
                for yuv in (0, 1):
                    if len(grp) == 1:
                        call_output_size(b, bd, ch, yuv)
                    call_workspace_bytes(b, bd, ch, yuv)
                    call_plan(b, bd, ch, yuv)
                for sample in SAMPLES:
                    call_dev_plan(b, bd, ch, sample)
                    for k in range(n_rects):  # a batch: frame j takes its rectangle (j + k)
                        call_roi_plan(b, [rects[i][(j + k) % len(rects[i])] for j, i in enumerate(grp)], bd, ch, sample)
    for i in range(n):
        w, h = frame_size(data[i])
        for cut in range(0, min(len(data[i]), header_size(data[i]) + 8) + 1):
            b = Batch([names[i]], [data[i][:cut]])
            call_output_size(b, 0, 0, 1)
            call_workspace_bytes(b, 0, 0, 1)
            call_plan(b, 0, 0, 0)
            call_dev_plan(b, 0, 0, 1)
            call_roi_plan(b, [(0, 0, w, h)], 0, 0, 1)
            call_roi_plan(b, [(2, 2, max(1, w // 2), max(1, h // 2))], 0, 0, 2)
    sys.stdout.flush()


if __name__ == "__main__":
    main()
