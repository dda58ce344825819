"""The dispatch matrix of the decoder's output stage (dec_out.hip): every cell of
geometry {roi=, roi= + size=, affine= + size=, perspective= + size=, the last three also with
interpolation="bicubic": the seven geometries of dec_out.hip} x colour {no ops, ops without a
contrast op, ops with one (the statistics pass)} x element type {float32, float16, bfloat16}, each
through the batched tail (a tail group: the kernels that read the group's tables) and through the
per-frame tail (the kernels that take the frame by value) in ONE render_model call over the
formatted-output tests' generated 21 x 37 streams.

A cell that launches another cell's kernel still runs, so every cell is compared BITWISE with the
chain the other tests pin: the float32 render WITHOUT ops (mean 0, std 1; test_decode_fmt_gpu,
test_decode_resample_gpu, test_decode_warp_gpu, test_decode_cubic_gpu, test_decode_persp_gpu), put
through tests/colour_ref.py, then scale, bias and .to(dtype) -- test_decode_colour_gpu's _base /
_want.  Outputs are 7 x 5, channel-first.

The bases of the four cells those last two modules pin were checked once with exactly the arguments
below, on both streams (frame 0: the tail group, frame 1: the per-frame tail): bitwise equal to
cubic_ref.resample of q's region, cubic_ref.warp, and persp_ref.render without and with WARP_CUBIC,
q from decode_batch's bytes through test_decode_warp_gpu's _q (8 bit, 444, RGB)."""
import numpy as np
import pytest

from test_decode_colour_gpu import FILL, _base, _check, _rot
from test_decode_fmt_gpu import MEAN, STD, _generate

pytestmark = pytest.mark.gpu

AFFINE = dict(affine=_rot(-30, 1.25, (30.0, 12.0), (7, 5)), size=(7, 5), fill=FILL, pad="fill")
# a homography that is no affine map (the denominator runs from 1.014 to 1.158 over the 7 x 5 output): the
# rotation above with a third row; the plan accepts it for the 21 x 37 frame
PERSPECTIVE = dict(perspective=np.concatenate([_rot(-30, 1.25, (30.0, 12.0), (7, 5)),
                                               np.array([[0.012, 0.016, 1.0]], np.float32)]),
                   size=(7, 5), fill=FILL, pad="fill")
GEOMETRY = {
    "roi": dict(roi=(3, 5, 5, 7)),
    "size": dict(roi=(3, 5, 17, 11), size=(7, 5)),
    "size-cubic": dict(roi=(3, 5, 17, 11), size=(7, 5), interpolation="bicubic"),
    "affine": AFFINE,
    "affine-cubic": dict(AFFINE, interpolation="bicubic"),
    "persp": PERSPECTIVE,
    "persp-cubic": dict(PERSPECTIVE, interpolation="bicubic"),
}
# per frame: [the batched tail's, the per-frame tail's]
COLOUR = {
    "none": None,
    "ops": [[("saturation", 0.4), ("brightness", 1.3)], [("brightness", 0.8), ("saturation", 1.6)]],
    "contrast": [[("brightness", 1.3), ("contrast", 1.7), ("saturation", 0.4)], [("contrast", 0.45), ("brightness", 1.1)]],
}
DTYPES = ("float32", "float16", "bfloat16")


@pytest.fixture(scope="module")
def store(gpu, ccmi_lib):
    """[21 x 37: the batched tail, 21 x 37 with a generic synthesis: the per-frame tail]"""
    from ccmi import decode
    st = decode.LatentStore([_generate(21, 37, 7), _generate(21, 37, 11, generic=True)])
    yield st
    st.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("colour", sorted(COLOUR))
@pytest.mark.parametrize("geometry", sorted(GEOMETRY))
def test_cell(store, geometry, colour, dtype):
    import torch
    from ccmi import decode
    dtype = getattr(torch, dtype)
    kw = dict(index=[0, 1], output_chroma_format=444, **GEOMETRY[geometry])
    base = _base(store, ("matrix", geometry), **kw)
    assert tuple(base.shape) == (2, 3, 7, 5)
    ops = COLOUR[colour]
    got = store.render_model(colour_ops=ops, mean=MEAN, std=STD, dtype=dtype, **kw)
    assert decode.last_tail_groups() == (1, 1)
    assert got.dtype == dtype and got.is_contiguous() and tuple(got.shape) == (2, 3, 7, 5)
    _check(got, base, ops or [[], []], (geometry, colour, dtype), mean=MEAN, std=STD, dtype=dtype)
