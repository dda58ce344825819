"""ccmi_msssim_f32 / ccmi_train_step_dist on a host without a GPU: every argument error is
CCMI_ERR_ARG with a message before any HIP call (the pointers below are never dereferenced), and
ccmi_msssim_workspace_bytes equals the formula of include/ccmi.h to the byte."""
import ctypes as C

import pytest

import msssim_ref as R


def _args(h=41, w=43, S=3, B=2, grad=False, sizes=None):
    from ccmi.metrics import MsssimArgs
    a = MsssimArgs()
    sizes = sizes or [(h, w)] * 3
    a.batch, a.n_planes, a.n_scales, a.clamp = B, 3, S, 1
    o = 0
    for p, (hh, ww) in enumerate(sizes):
        a.h[p], a.w[p] = hh, ww
        a.x_off[p], a.x_pitch[p], a.x_sub[p] = o, ww, 1
        o += hh * ww
    a.x, a.x_stride, a.y, a.y_stride = 0x1000, o, 0x1000, o
    for i, v in enumerate(R.default_weights(S)):
        a.weights[i] = v
    for p in range(3):
        a.channel_weights[p] = 1 / 3
    a.alpha_mse, a.beta_ms = 0.3, 0.7
    a.out = 0x1000
    a.grad = 0x1000 if grad else None
    a.workspace, a.workspace_bytes = 0x1000, 1 << 40
    return a


def _refused(ccmi_lib, a, word):
    import ccmi
    from ccmi.metrics import _bind
    rc = _bind().ccmi_msssim_f32(C.byref(a), None)
    assert rc == ccmi.ERR_ARG, (rc, word)
    assert word in ccmi.last_error(), (word, ccmi.last_error())


def test_argument_errors_are_reported_before_any_hip_call(ccmi_lib):
    a = _args()
    a.out = None
    _refused(ccmi_lib, a, "out is null")
    a = _args()
    a.x = None
    _refused(ccmi_lib, a, "null")
    a = _args(h=40, w=43, S=3)  # 40 -> 20 -> 10
    _refused(ccmi_lib, a, "plane 0 is 10 x 11 at scale 2")
    a = _args(sizes=[(41, 43), (41, 43), (20, 43)], S=2)
    _refused(ccmi_lib, a, "plane 2 is 10 x 22 at scale 1")
    a = _args(h=160, w=161, S=5)
    _refused(ccmi_lib, a, "scale 4")
    for bad in (-0.1, float("nan"), float("inf")):
        a = _args()
        a.weights[1] = bad
        _refused(ccmi_lib, a, "weights[1]")
        a = _args()
        a.channel_weights[2] = bad
        _refused(ccmi_lib, a, "channel_weights[2]")
        a = _args()
        a.beta_ms = bad
        _refused(ccmi_lib, a, "beta_ms")
    a = _args()
    a.workspace_bytes = R.workspace_bytes(2, [(41, 43)] * 3, 3, False) - 1
    _refused(ccmi_lib, a, "workspace of %d bytes" % R.workspace_bytes(2, [(41, 43)] * 3, 3, False))
    a = _args()
    a.workspace = None
    _refused(ccmi_lib, a, "workspace")
    for sub in (0, 3, -1):
        a = _args()
        a.x_sub[1] = sub
        _refused(ccmi_lib, a, "x_sub[1]")
    a = _args()
    a.n_scales = 6
    _refused(ccmi_lib, a, "n_scales")
    a = _args()
    a.n_planes = 4
    _refused(ccmi_lib, a, "n_planes")
    a = _args()
    a.batch = 0
    _refused(ccmi_lib, a, "batch")
    a = _args()
    a.y_stride = 5
    _refused(ccmi_lib, a, "y_stride")
    from ccmi.metrics import _bind
    assert _bind().ccmi_msssim_f32(None, None) == 1


@pytest.mark.parametrize("grad", [False, True])
def test_workspace_formula_to_the_byte(ccmi_lib, grad):
    from ccmi.metrics import _bind
    L = _bind()
    seen = set()
    for c in R.CASES:
        for B in (1, c.B, 7, 960):
            a = _args(S=c.S, B=B, grad=grad, sizes=c.sizes)
            want = R.workspace_bytes(B, c.sizes, c.S, grad)
            assert L.ccmi_msssim_workspace_bytes(C.byref(a)) == want, (c.name, B)
            seen.add(want)
    assert len(seen) > 20
    a = _args(h=1280, w=720, S=5, B=960, grad=grad)
    assert L.ccmi_msssim_workspace_bytes(C.byref(a)) == R.workspace_bytes(960, [(1280, 720)] * 3, 5, grad)
    a = _args(h=40, w=43, S=3)
    assert L.ccmi_msssim_workspace_bytes(C.byref(a)) == 0  # invalid shapes have no workspace


def test_train_dist_errors_and_workspace(ccmi_lib):
    """ccmi_train_workspace_bytes_dist = the step's own plan, a [B][4] row, the stage's workspace with
    its gradient part; dist = NULL is ccmi_train_workspace_bytes; dist with grad_raw is refused."""
    import ccmi
    import torch
    from ccmi import train as T
    from ccmi.metrics import Distortion
    L = T._bind()
    al = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for yuv420, S in ((False, 5), (True, 4)):
        arch = T.Arch(176, 208)
        a = T.TrainArgs()
        a.batch, a.n_grids = 2, arch.n_grids
        for i, (h, w) in enumerate(arch.sizes):
            a.h[i], a.w[i] = h, w
        a.dim_arm, a.n_hidden = arch.dim_arm, arch.n_hidden
        a.ups_k, a.n_ups, a.pre_k, a.n_pre = arch.ups_k, arch.n_grids - 1, arch.pre_k, arch.n_grids - 1
        a.n_syn_layers = len(arch.layers)
        for i, (n, k, r, nl) in enumerate(arch.layers):
            a.syn[i] = ccmi.SynLayer(n, k, int(r), int(nl))
        a.gain, a.yuv420 = arch.gain, int(yuv420)
        a.latent_stride, a.param_stride = arch.n_latents, L.ccmi_train_param_count(C.byref(a))
        sizes = [(176, 208)] + [(88, 104) if yuv420 else (176, 208)] * 2
        a.target_stride = sum(h * w for h, w in sizes)
        base = L.ccmi_train_workspace_bytes(C.byref(a))
        assert base > 0
        d = Distortion(0.0, 1.0, n_scales=S).train_struct(yuv420)
        assert L.ccmi_train_workspace_bytes_dist(C.byref(a), None) == base
        assert L.ccmi_train_workspace_bytes_dist(C.byref(a), C.byref(d)) == \
            al(base) + al(16 * 2) + R.workspace_bytes(2, sizes, S, True)
        a.latent = a.params = a.target = a.grad_raw = 0x1000
        a.workspace, a.workspace_bytes = 0x1000, 1 << 40
        assert L.ccmi_train_step_dist(C.byref(a), C.byref(d), None) == ccmi.ERR_ARG
        assert "grad_raw" in ccmi.last_error()
        a.grad_raw = None
        if yuv420:  # five scales do not fit a chroma plane of 88 x 104
            d5 = Distortion(0.0, 1.0, n_scales=5).train_struct(yuv420)
            assert L.ccmi_train_workspace_bytes_dist(C.byref(a), C.byref(d5)) == 0
            assert L.ccmi_train_step_dist(C.byref(a), C.byref(d5), None) == ccmi.ERR_ARG
            assert "plane 1" in ccmi.last_error() and "scale 4" in ccmi.last_error()
        a.workspace_bytes = al(base) + 256
        assert L.ccmi_train_step_dist(C.byref(a), C.byref(d), None) == ccmi.ERR_ARG
        assert "workspace" in ccmi.last_error()
