"""GPU tests of the stem max-pool passes on caller tensors: ``bn_relu_maxpool_kernel`` (``neraf_debug_maxpool_fwd``) and
``maxpool_bwd_gather_kernel`` (``neraf_debug_maxpool_bwd``).

Forward.  The input is small integers in fp16 (-8 .. 8), so ties inside a window are the rule; BatchNorm runs in eval mode with
gamma = 1, beta = 0.25, running mean 0 and running variance 1: scale s = 1 / sqrt(1 + 1e-5) > 0 and shift 0.25, the activation
max(x s + 0.25, 0) is monotone in x, positive for x >= 0 and zero for x <= -1, and x s + 0.25 is at least 0.25 away from zero for
every integer x.  The routing table is therefore EXACT on the host: the first maximum of x over the window's taps inside the image in
(dz, dy, dx) order, or 255 where that maximum is negative; it must match for every window and channel.  The pooled value must lie
within one fp16 ulp of the float64 evaluation.  din = 4 puts every window on a border; din = 6 and 10 have an odd number of windows
per axis, 10 and 16 more than one workgroup.

Backward.  g is small integers, so the fp32 sum of the <= 8 contributions of a voxel is exact in any order and the result must be
BIT-EQUAL to a host scatter of g through the table, rows [din^3, rows_pad) zero and nothing written beyond."""
import ctypes as C

import numpy as np
import pytest
import torch

from neraf_amd import synth

pytestmark = pytest.mark.gpu

DINS = [4, 6, 10, 16]
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


def _dout(din):
    return (din - 1) // 2 + 1


_HOST = {}


def _host(din, lo=-8, hi=8):
    """Integer input [din^3][64] and the exact expectations of the forward, computed once and shared (never modified)."""
    key = (din, lo, hi)
    if key not in _HOST:
        dout = _dout(din)
        u = synth.uniform(f"maxpool.x.{din}.{lo}.{hi}", (din, din, din, 64), 0.0, 1.0)
        x = np.minimum(np.floor(u * (hi - lo + 1)) + lo, hi).astype(np.float64)
        xp = np.full((din + 2, din + 2, din + 2, 64), -np.inf)
        xp[1:-1, 1:-1, 1:-1] = x
        taps = np.stack([xp[dz:dz + 2 * dout:2, dy:dy + 2 * dout:2, dx:dx + 2 * dout:2]
                         for dz in range(3) for dy in range(3) for dx in range(3)])          # [27][dout][dout][dout][64], tap order
        first = taps.argmax(0)                                                               # numpy returns the FIRST maximum
        best = taps.max(0)
        arg = np.where(best < 0, 255, first).astype(np.uint8).reshape(dout ** 3, 64)
        s = 1.0 / np.sqrt(1.0 + 1e-5)
        val = np.maximum(best * s + 0.25, 0.0).reshape(dout ** 3, 64)
        _HOST[key] = dict(x=x.reshape(din ** 3, 64).astype(np.float16), arg=arg, val=val)
    return _HOST[key]


def _forward(lib, h, dev, din, x16):
    dout = _dout(din)
    xd = torch.from_numpy(x16).to(dev)
    par = [torch.full((64,), v, dtype=torch.float32, device=dev) for v in (1.0, 0.25, 0.0, 1.0)]      # gamma, beta, mean, var
    bn5 = (C.c_void_p * 5)(None, *[p.data_ptr() for p in par])
    out = torch.full((dout ** 3 + GUARD_ROWS, 64), CANARY, dtype=torch.int16, device=dev)
    arg = torch.full((dout ** 3 + GUARD_ROWS, 64), 0xA5, dtype=torch.uint8, device=dev)
    rc = lib.neraf_debug_maxpool_fwd(h, xd.data_ptr(), bn5, 1, din, out.data_ptr(), arg.data_ptr(), _stream())
    assert rc == 0, lib.neraf_last_error(h)
    torch.cuda.synchronize()
    out, arg = out.cpu().numpy(), arg.cpu().numpy()
    assert (out[dout ** 3:] == CANARY).all() and (arg[dout ** 3:] == 0xA5).all(), "written beyond the last window"
    return out[:dout ** 3].view(np.float16), arg[:dout ** 3]


def _ulp16(v):
    """spacing of fp16 at |v| (float64 array)"""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return 2.0 ** (e - 10)


@pytest.mark.parametrize("din", DINS)
def test_forward_routing_table_exact_and_values(lib_h, dev, din):
    lib, h = lib_h
    ref = _host(din)
    out, arg = _forward(lib, h, dev, din, ref["x"])
    bad = arg != ref["arg"]
    assert not bad.any(), f"din={din}: {int(bad.sum())} of {bad.size} routing entries differ, first at {np.argwhere(bad)[0]}"
    err = np.abs(out.astype(np.float64) - ref["val"])
    print(f"din={din}: max |value - float64| = {err.max():.3e} (largest bound {_ulp16(ref['val']).max():.3e})")
    assert (err <= _ulp16(ref["val"])).all(), f"din={din}: pooled value more than one fp16 ulp from the float64 evaluation"
    assert ((arg == 255) == (out == 0)).all()


def test_forward_all_negative_input(lib_h, dev):
    lib, h = lib_h
    ref = _host(6, -8, -1)
    assert (ref["arg"] == 255).all()
    out, arg = _forward(lib, h, dev, 6, ref["x"])
    assert (arg == 255).all() and (out.view(np.int16) == 0).all()


def _host_scatter(arg, g16, din):
    """dpost [rows_pad][64] fp16: every window's g goes to the input voxel its table entry names (exact: small integers)."""
    dout = _dout(din)
    rows_pad = (din ** 3 + 127) // 128 * 128
    acc = np.zeros((rows_pad, 64), np.float32)
    o = np.arange(dout ** 3)
    oz, oy, ox = o // (dout * dout), (o // dout) % dout, o % dout
    ch = np.arange(64)[None, :].repeat(dout ** 3, 0)
    t = arg.astype(np.int64)
    ok = t != 255
    iz = 2 * oz[:, None] + t // 9 - 1
    iy = 2 * oy[:, None] + (t // 3) % 3 - 1
    ix = 2 * ox[:, None] + t % 3 - 1
    assert ((iz[ok] >= 0) & (iz[ok] < din) & (iy[ok] >= 0) & (iy[ok] < din) & (ix[ok] >= 0) & (ix[ok] < din)).all(), "table names a tap outside"
    vox = (iz * din + iy) * din + ix
    np.add.at(acc, (vox[ok], ch[ok]), g16.astype(np.float32)[ok])
    return acc.astype(np.float16)


def _backward(lib, h, dev, din, arg, g16):
    rows_pad = (din ** 3 + 127) // 128 * 128
    buf = torch.full((rows_pad + GUARD_ROWS, 64), CANARY, dtype=torch.int16, device=dev)
    ad, gd = torch.from_numpy(arg).to(dev), torch.from_numpy(g16).to(dev)
    rc = lib.neraf_debug_maxpool_bwd(h, ad.data_ptr(), gd.data_ptr(), din, buf.data_ptr(), _stream())
    assert rc == 0, lib.neraf_last_error(h)
    torch.cuda.synchronize()
    buf = buf.cpu().numpy()
    assert (buf[rows_pad:] == CANARY).all(), "written beyond rows_pad"
    assert (buf[din ** 3:rows_pad] == 0).all(), "rows [din^3, rows_pad) are not zero"
    return buf[:rows_pad]


def _g(din):
    dout = _dout(din)
    u = synth.uniform(f"maxpool.g.{din}", (dout ** 3, 64), 0.0, 1.0)
    return (np.floor(u * 9) - 4).clip(-4, 4).astype(np.float16)


@pytest.mark.parametrize("din", DINS)
def test_backward_bit_equal_to_host_scatter(lib_h, dev, din):
    lib, h = lib_h
    ref = _host(din)
    _, arg = _forward(lib, h, dev, din, ref["x"])            # the table the forward wrote (equal to ref["arg"], tested above)
    g = _g(din)
    got = _backward(lib, h, dev, din, np.ascontiguousarray(arg), g)
    want = _host_scatter(ref["arg"], g, din)
    bad = got != want.view(np.int16)
    assert not bad.any(), f"din={din}: {int(bad.sum())} gradient elements differ, first at {np.argwhere(bad)[0]}"


def test_backward_one_voxel_wins_all_eight_windows_and_empty_table(lib_h, dev):
    lib, h = lib_h
    din, dout = 6, 3
    g = _g(din)
    arg = np.full((dout ** 3, 64), 255, np.uint8)
    # input voxel (1, 1, 1) lies in the windows (0..1)^3: through tap d = +1 (index 2) of window 0 and d = -1 (index 0) of window 1
    for oz in (0, 1):
        for oy in (0, 1):
            for ox in (0, 1):
                arg[(oz * dout + oy) * dout + ox] = (2 - 2 * oz) * 9 + (2 - 2 * oy) * 3 + (2 - 2 * ox)
    got = _backward(lib, h, dev, din, arg, g)
    want = _host_scatter(arg, g, din)
    assert np.array_equal(got, want.view(np.int16))
    v = (1 * din + 1) * din + 1
    assert np.array_equal(got[v].view(np.float16).astype(np.float32),
                          sum(g[(oz * dout + oy) * dout + ox].astype(np.float32) for oz in (0, 1) for oy in (0, 1) for ox in (0, 1)))
    assert (np.delete(got, v, axis=0) == 0).all()
    empty = np.full((dout ** 3, 64), 255, np.uint8)
    assert (_backward(lib, h, dev, din, empty, g) == 0).all()
