"""GPU test of the stem convolution launch alone (``neraf_debug_stem_conv``: ``gemm_f16_nt_pipe_kernel<128, 64, 3, 2, 5>``, the
tap-per-chunk loader with per-thread tap counters, validity masks and 32-bit base offsets) against torch's ``conv3d`` on the CPU in
float64.

Inputs and weights are integers in {-1, 0, 1}: a result element is a sum of at most 125 taps x 7 channels = 875 terms, |.| <= 875 <
2048, exact in fp16 and in the fp32 accumulators whatever the summation order -- so the fp16 result must EQUAL the reference.  The
column sums (the fused BatchNorm statistics) are sums of integers below 2^24 (4096 rows x 875 at most) and must equal the reference's
exactly too; the sums of squares are non-negative fp32 sums of up to M terms in an order the hardware chooses, bound (M - 1) 2^-24
relative.  (The reference's maximum is asserted below; it is 60 / 84 / 91 for the three sizes.)

The eighth stored channel holds the sentinel 3 everywhere: only the 7 real weight channels may count.  din = 8 gives 64 result rows
in one 128-row tile, every row touching the padding; din = 16 gives 512 rows with interior rows that see all 125 taps; din = 32 has
32 tiles.  Rows [M, Mpad) must be zero, and canary rows before and after the buffer must stay intact."""
import ctypes as C

import numpy as np
import pytest
import torch

from neraf_amd import synth

pytestmark = pytest.mark.gpu

CANARY = 0x7BCD
GUARD_ROWS = 128


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib_h(dev):
    from neraf_amd import _lib
    return _lib.load(), _lib.ctx(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tern(tag, shape):
    return (np.minimum(np.floor(synth.uniform(tag, shape, 0.0, 1.0) * 3.0), 2.0) - 1.0).astype(np.float64)


_HOST = {}


def _host(din):
    """Integer operands and the float64 reference, computed once per size and never modified."""
    if din not in _HOST:
        x = np.empty((din, din, din, 8))
        x[..., :7] = _tern(f"stemconv.x.{din}", (din, din, din, 7))
        x[..., 7] = 3.0
        w = _tern(f"stemconv.w.{din}", (64, 7, 5, 5, 5))
        xt = torch.from_numpy(x[..., :7]).permute(3, 0, 1, 2)[None]
        y = torch.nn.functional.conv3d(xt, torch.from_numpy(w), stride=2, padding=2)[0]      # [64][dout]^3, float64
        y = y.permute(1, 2, 3, 0).reshape(-1, 64).numpy()
        assert np.abs(y).max() < 2048
        _HOST[din] = dict(x=x.reshape(-1, 8).astype(np.float16), w=w.reshape(64, 7, 125).astype(np.float32), y=y)
    return _HOST[din]


@pytest.mark.parametrize("din", [8, 16, 32])
def test_stem_conv_equals_conv3d(lib_h, dev, din):
    lib, h = lib_h
    ref = _host(din)
    M = (din // 2) ** 3
    Mpad = (M + 127) // 128 * 128
    xd = torch.from_numpy(ref["x"]).to(dev)
    wd = torch.from_numpy(ref["w"]).to(dev)
    buf = torch.full((GUARD_ROWS + Mpad + GUARD_ROWS, 64), CANARY, dtype=torch.int16, device=dev)
    sums = torch.full((3, 128), 7.0, dtype=torch.float32, device=dev)        # third row: guard
    rc = lib.neraf_debug_stem_conv(h, din, 7, xd.data_ptr(), wd.data_ptr(), buf[GUARD_ROWS:].data_ptr(), sums.data_ptr(), _stream())
    assert rc == 0, lib.neraf_last_error(h)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:GUARD_ROWS] == CANARY).all() and (out[GUARD_ROWS + Mpad:] == CANARY).all(), "written outside [0, Mpad) rows"
    got = out[GUARD_ROWS:GUARD_ROWS + Mpad].view(np.float16).astype(np.float64)
    assert (got[M:] == 0).all(), "rows [M, Mpad) must be zero"
    bad = got[:M] != ref["y"]
    assert not bad.any(), f"din={din}: {int(bad.sum())} of {bad.size} elements differ, first at row/col {np.argwhere(bad)[0]}"
    s = sums.cpu().numpy().astype(np.float64)
    assert (s[2] == 7.0).all()
    np.testing.assert_array_equal(s[0, :64], ref["y"].sum(0))
    sq = (ref["y"] ** 2).sum(0)
    assert (np.abs(s[1, :64] - sq) <= (M - 1) * 2.0 ** -24 * sq).all()
    assert (s[:2, 64:] == 0).all()
