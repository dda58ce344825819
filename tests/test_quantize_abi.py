"""ccmi_quantize_f32's argument checks, which run before any device call: n = 0 is accepted and
writes nothing, and a temperature of 0 is refused by the three types that divide by it and
accepted by the others.  No kernel is launched here (CPU hosts have no HIP device): every accepted
call has n = 0."""
import ctypes as C

import pytest

import quant_ref as Q


@pytest.fixture(scope="module")
def qf(ccmi_lib):
    f = ccmi_lib.ccmi_quantize_f32
    f.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    return f


def _buffers():
    return [(C.c_float * 4)(*([-12345.0] * 4)) for _ in range(4)]


@pytest.mark.parametrize("qtype", Q.QTYPES)
def test_n_zero_is_accepted_and_writes_nothing(qtype, qf):
    from ccmi.train import Q_TYPES
    x, nz, y, dy = _buffers()
    for noise, d in ((nz, dy), (None, None)):
        assert qf(x, 0, Q_TYPES[qtype], 0.3, noise, y, d, None) == 0
    assert list(y) == [-12345.0] * 4 and list(dy) == [-12345.0] * 4


@pytest.mark.parametrize("qtype", Q.QTYPES)
def test_temperature_zero_is_refused_where_it_is_read(qtype, qf):
    import ccmi
    from ccmi.train import Q_TYPES
    x, nz, y, dy = _buffers()
    for T in (0.0, -0.1, float("nan")):
        rc = qf(x, 0, Q_TYPES[qtype], T, nz, y, dy, None)
        if qtype in Q.READS_T:
            assert rc != 0 and "temperature" in ccmi.last_error(), (qtype, T)
        else:
            assert rc == 0, (qtype, T, ccmi.last_error())
    assert list(y) == [-12345.0] * 4 and list(dy) == [-12345.0] * 4


def test_other_argument_errors(qf):
    import ccmi
    x, nz, y, dy = _buffers()
    assert qf(None, 0, 2, 0.3, nz, y, dy, None) != 0 and "null" in ccmi.last_error()
    assert qf(x, 0, 2, 0.3, nz, None, dy, None) != 0 and "null" in ccmi.last_error()
    assert qf(x, -1, 2, 0.3, nz, y, dy, None) != 0
    assert qf(x, 2 ** 31, 2, 0.3, nz, y, dy, None) != 0 and "2^31" in ccmi.last_error()
    for bad in (-1, 6):
        assert qf(x, 0, bad, 0.3, nz, y, dy, None) != 0 and "type" in ccmi.last_error()
