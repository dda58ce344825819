"""The equivalence ccmi/decode.py relies on: decode_batch_model and LatentStore.render_model reach every
formatted call through the *_mix entry points with the absent stages NULL, which ccmi.h defines to be the
narrower call.  Here each of the seven formatted rungs (fmt, rs, warp, col, flt, tone, mix), from both
sources, is given exactly the stages its own entry point can express; the public call is compared with that
entry point called directly through decode._bind(): the same ctypes descriptors (the module's own _warp,
_colour, _filter, _tone, _mix, _resample and _model_fmt), the workspace size of the rung's own _plan, the
test's own output buffer.

No tolerance: the two requests are identical, so the bits, the tail groups, the planned geometry and the
workspace bytes are equal or something is wrong.

Three frames of the smallest committed stream (class D, 416 x 240, 4:2:0), regions of 64 x 48 at even origins,
size=(24, 32), the middle frame mirrored, float32 and bfloat16."""
import ctypes as C

import numpy as np
import pytest

from test_decode_fmt_gpu import MEAN, STD, _sentinel_canvas
from test_decode_resample_abi import _first

pytestmark = pytest.mark.gpu

N = 3
ROIS = [(0, 0, 64, 48), (100, 60, 64, 48), (352, 192, 64, 48)]
SIZE = (24, 32)
MIRROR = [False, True, False]
RUNGS = ("fmt", "rs", "warp", "col", "flt", "tone", "mix")


def _keywords(rung):
    """The stages of a rung, as the keywords of the public calls."""
    from ccmi import decode
    mats = np.stack([decode.affine_matrix(SIZE, (100, 80), 0.3, 0.5), decode.affine_matrix(SIZE, (208, 120), -0.2, 0.25, True),
                     decode.affine_matrix(SIZE, (10, 10))])  # the last one reaches outside the frame: fill
    col = dict(colour_ops=[[("brightness", 1.2), ("contrast", 0.8)], [], [("matrix", decode.hue_matrix(0.1)), ("saturation", 1.3)]])
    blur = dict(blur=[decode.gaussian_taps(1.0, 5), None, decode.gaussian_taps(0.7, 3)])
    tone = dict(tone_ops=[[("posterize", 4), ("autocontrast", None)], [("equalize", None)], [("sharpness", 1.5)]])
    region = dict(roi=ROIS, size=SIZE)
    return {"fmt": dict(roi=ROIS),
            "rs": region,
            "warp": dict(affine=mats, size=SIZE),
            "col": dict(region, **col),
            "flt": dict(affine=mats, size=SIZE, solarize=[0.5, None, 0.9], **col, **blur),
            "tone": dict(region, **col, **tone, **blur),
            "mix": dict(region, **col, **tone, **blur, erase=[[(3, 2, 9, 7, 0.25), (10, 10, 6, 6, 0.0, 1.0)], None,
                                                               [(0, 0, 5, 5, (1.0, -2.0, 3.0))]],
                        erase_seed=5, mix=[(1, 0.3), None, (0, (2, 2, 9, 9))])}[rung]


@pytest.fixture(scope="module")
def streams():
    return [_first("D-")] * N


@pytest.fixture(scope="module")
def store(streams):
    from ccmi import decode
    st = decode.LatentStore(streams)
    yield st
    st.close()


def _int_view(t):
    import torch
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("source", ["streams", "store"])
@pytest.mark.parametrize("rung", RUNGS)
def test_the_mix_entry_point_is_the_rungs_own_call(streams, store, rung, source):
    import torch
    for dtype in (torch.float32, torch.bfloat16):
        _compare(streams, store, rung, source, dtype)


def _compare(streams, store, rung, source, dtype):
    import torch
    from ccmi import decode
    kw = _keywords(rung)
    L = decode._bind()

    # the public call: through the *_mix pair
    if source == "streams":
        got = decode.decode_batch_model(streams, dtype=dtype, mean=MEAN, std=STD, mirror=MIRROR, **kw)
    else:
        got = store.render_model(dtype=dtype, mean=MEAN, std=STD, mirror=MIRROR, **kw)
    groups = decode.last_tail_groups()

    # the same descriptors, built once more by the module's own marshalling
    interp = decode._interp("bilinear", False)
    warp, keep_w = decode._warp(kw.get("affine"), N, kw.get("size"), kw.get("roi"), "fill", 0.0, interp)
    col, keep_c = decode._colour(kw.get("colour_ops"), N)
    flt, keep_f = decode._filter(kw.get("blur"), kw.get("solarize"), N)
    tone, keep_t = decode._tone(kw.get("tone_ops"), N)
    mx, keep_m = decode._mix(kw.get("erase"), kw.get("erase_seed"), kw.get("mix"), N)
    rs = decode._resample(kw["size"], interp) if "size" in kw and warp is None else None
    fmt, keep = decode._model_fmt(N, "rgb", MEAN, STD, dtype, MIRROR)
    if source == "streams":
        marshalled, sp, ln = decode._marshal(streams)
        src, name = decode._stream_source(sp, ln), "ccmi_decode_batch_dev_" + rung
        rects = None if warp is not None else decode._rects(kw.get("roi"), streams, N)
    else:
        m, idx, rects = store._frames(None, None if warp is not None else kw.get("roi"))
        src, name = store._source(idx), "ccmi_latents_render_" + rung
    head = src[2]

    # exactly what the rung's own prototype takes between the format and the outputs
    ref = lambda s: None if s is None else C.byref(s)  # noqa: E731
    have = {"fmt": (), "rs": (rs,), "warp": (warp,), "col": (rs, warp, col), "flt": (rs, warp, col, flt),
            "tone": (rs, warp, col, tone, flt), "mix": (rs, warp, col, tone, flt, mx)}[rung]
    given = [s for s in (rs, warp, col, tone, flt, mx) if s is not None]
    assert all(any(s is h for h in have) for s in given), "the rung was given a stage its entry point cannot take"
    stages = [ref(s) for s in have]
    roi_arg = [] if rung == "warp" else [rects]
    window_arg = [] if rung in ("fmt", "rs") else [None]

    # the two plans: the rung's own, and the *_mix one the module makes
    geom, need = (decode.FrameGeom * N)(), C.c_size_t(0)
    probe = decode.TensorFmt.from_buffer_copy(fmt)
    decode.check(getattr(L, name + "_plan")(*head, N, *roi_arg, 0, 0, C.byref(probe), *stages, geom, None, *window_arg,
                                            C.byref(need)))
    sink = decode._Sink(N, rects, rs, warp, col, tone, flt, mx)
    geom_mix, need_mix = decode._plan_model(src, sink, fmt, 0, 0)
    fields = [k for k, _ in decode.FrameGeom._fields_]
    assert [[getattr(g, k) for k in fields] for g in geom] == [[getattr(g, k) for k in fields] for g in geom_mix]
    assert need.value == need_mix
    h, w = geom[0].height, geom[0].width
    assert (h, w) == ((48, 64) if rung == "fmt" else SIZE) and tuple(got.shape) == (N, 3, h, w)

    # the rung's own run, into this test's buffer and a workspace of its own plan's size
    buf, pattern = _sentinel_canvas((N, 3, h, w), dtype)
    fmt.stride_c, fmt.stride_y, fmt.stride_x = (int(s) for s in buf[0].stride())
    op = (C.c_void_p * N)(*[buf[i].data_ptr() for i in range(N)])
    cap = (C.c_size_t * N)(*[(N - i) * 3 * h * w * buf.element_size() for i in range(N)])
    ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device="cuda")
    decode.check(getattr(L, name)(*head, N, *roi_arg, op, cap, C.byref(fmt), *stages, 0, 0, ws.data_ptr(), ws.numel(),
                                  torch.cuda.current_stream().cuda_stream))
    assert decode.last_tail_groups() == groups
    torch.cuda.synchronize()
    assert not bool((_int_view(buf) == pattern).all(dim=(1, 2, 3)).any()), "a frame was not written"
    assert torch.equal(_int_view(got), _int_view(buf))
