"""The resampling steps 3a-3c of the ccmi_resample contract (include/ccmi.h) in numpy float32, one
rounded operation at a time: the reference of tests/test_decode_resample_gpu.py, pinned by
tests/test_decode_resample_ref.py against torch's antialiased bilinear in float64.  Nothing here
calls the library."""
import numpy as np

F32 = np.float32


def axis_weights(I, O):
    """Per output index i of an axis resampled from extent I to O: (j0, float32 weights of the
    taps j0 .. j0 + len - 1).  u(i, j) = max(0, 2 D - |(2 j + 1) O - (2 i + 1) I|), D = max(I, O);
    w = float32(u) / float32(U), one float32 division."""
    D = max(I, O)
    j = np.arange(I, dtype=np.int64)
    out = []
    for i in range(O):
        u = np.maximum(0, 2 * D - np.abs((2 * j + 1) * O - (2 * i + 1) * I))
        nz = np.nonzero(u)[0]
        j0, j1 = int(nz[0]), int(nz[-1])
        assert np.all(u[j0: j1 + 1] > 0), "the taps are one contiguous run"
        U = int(u.sum())
        w = u[j0: j1 + 1].astype(F32) / F32(U)
        assert w.dtype == F32
        out.append((j0, w))
    return out


def max_taps(I, O):
    return max(len(w) for _, w in axis_weights(I, O))


def resample(q, oh, ow):
    """q: [C, h, w] float32 -> [C, oh, ow] float32: the horizontal pass over every region row, then
    the vertical pass; each sum starts from 0 and runs over the taps ascending, every product and
    every sum one float32 operation."""
    q = np.ascontiguousarray(q)
    assert q.dtype == F32 and q.ndim == 3
    C, h, w = q.shape
    t = np.zeros((C, h, ow), F32)
    for i, (j0, ws) in enumerate(axis_weights(w, ow)):
        acc = np.zeros((C, h), F32)
        for k, wk in enumerate(ws):
            acc = acc + wk * q[:, :, j0 + k]
            assert acc.dtype == F32
        t[:, :, i] = acc
    r = np.zeros((C, oh, ow), F32)
    for i, (j0, ws) in enumerate(axis_weights(h, oh)):
        acc = np.zeros((C, ow), F32)
        for k, wk in enumerate(ws):
            acc = acc + wk * t[:, j0 + k, :]
            assert acc.dtype == F32
        r[:, i, :] = acc
    return r
