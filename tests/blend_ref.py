"""Reference of the blend stage (ccmi_blend; step 3b of the contract in include/ccmi.h) in torch CPU float32
operations, one per product and sum, on top of tests/mix_ref.py for steps 4, 4e and 4m.  A helper: no tests in
it.  tests/test_decode_blend_ref.py pins it to an independent idiom on the CPU, tests/test_decode_blend_gpu.py
compares the kernel with it.

A frame is a float32 tensor [3, oh, ow]: y_c(i, k) of the contract, the staged frame before step 4.  A blend
list is [(source, weight), ...]: z = w_0 y^{s_0}, then z = z + (w_t y^{s_t}) for t ascending; a weight is
rounded to float32 first, as the call's marshalling rounds it."""
import numpy as np
import torch

import mix_ref


def weighted_sum(ys, terms):
    """step 3b of one frame with terms: every product rounded before its sum, in the terms' order"""
    z = None
    for s, w in terms:
        y = ys[int(s)]
        assert y.dtype == torch.float32 and y.dim() == 3
        p = y.mul(float(np.float32(w)))
        z = p if z is None else z.add(p)
    return z


def batch(ys, scale, bias, blend=None, silent=None, erases=None, seeds=None, mixes=None):
    """Steps 3b, 4, 4e and 4m of a call: ys the frames' staged y, blend / silent as blend= / silent= of the
    *_model calls, the rest as mix_ref.batch takes it -> (frames, erased): the float32 frames before step 5 of
    the frames that are not silent, in call order, and mix_ref's Erased of every frame.  A source enters as
    its y (its own list does not); a partner enters with its own sum, which is what mix_ref.batch does with
    the frames handed to it."""
    n = len(ys)
    blend = blend or [None] * n
    silent = silent or [False] * n
    assert len(blend) == n and len(silent) == n
    zs = [weighted_sum(ys, blend[j]) if blend[j] else ys[j] for j in range(n)]
    out, erased = mix_ref.batch(zs, scale, bias, erases, seeds, mixes)
    return [out[j] for j in range(n) if not silent[j]], erased
