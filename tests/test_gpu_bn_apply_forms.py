"""GPU test of the two forms of the forward BatchNorm pass (``neraf_debug_bn_apply``): form 1, the tile kernel that tensors
of 65536 16-byte chunks or more run on (``bn_apply_tile_kernel``), against form 0, the small-launch kernel (``bn_apply_kernel``), BIT FOR BIT --
the activations and the published mean / biased variance.

Cases: M in {1, 63, 64, 65, 1000} with Mpad the next multiple of 128, C in {64, 128, 256, 512}, {no second operand, residual,
bn(downsample)} x {relu on, off}, train-mode statistics (replicated accumulators, 1 to 16 replicas) and eval-mode running statistics.
Every result buffer lies between two guard regions filled with a sentinel: rows [M, Mpad) must be zero, and nothing may be written
in front of row 0 or at / beyond row Mpad."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from neraf_amd import synth

pytestmark = pytest.mark.gpu

GUARD_ROWS = 128
CANARY = 0x7BCD                      # fp16 bit pattern of 63904: |bn(x)| + |bn_r(x)| of these inputs stays far below it
STRIDE = 1024                        # floats between statistic replicas
REP = {1: 1, 63: 1, 64: 2, 65: 4, 1000: 16}


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


def _replicated_stats(x16, rep, cpad):
    """[rep][2][cpad] column sums / sums of squares of x (fp32), rows dealt to the replicas round robin, replicas STRIDE floats apart."""
    M, Cc = x16.shape
    st = np.zeros((rep, STRIDE), np.float32)
    x = x16.astype(np.float32)
    for r in range(rep):
        part = x[r::rep]
        st[r, :Cc] = part.sum(0, dtype=np.float32)
        st[r, cpad:cpad + Cc] = (part * part).sum(0, dtype=np.float32)
    return st


class Operand:
    """One BatchNorm input on the device: x, its replicated statistics and affine / running parameters."""

    def __init__(self, tag, M, Cc, rep, dev):
        self.cpad = (Cc + 127) // 128 * 128
        x = synth.uniform(f"bn_forms.{tag}.x.{M}.{Cc}", (M, Cc), -2.0, 2.0).astype(np.float16)
        self.x = torch.from_numpy(x).to(dev)
        self.stats = torch.from_numpy(_replicated_stats(x, rep, self.cpad)).to(dev)
        self.gamma = torch.from_numpy(synth.uniform(f"bn_forms.{tag}.gamma.{Cc}", (Cc,), 0.5, 1.5)).to(dev)
        self.beta = torch.from_numpy(synth.uniform(f"bn_forms.{tag}.beta.{Cc}", (Cc,), -0.5, 0.5)).to(dev)
        self.rmean = torch.from_numpy(synth.uniform(f"bn_forms.{tag}.rmean.{Cc}", (Cc,), -0.3, 0.3)).to(dev)
        self.rvar = torch.from_numpy(synth.uniform(f"bn_forms.{tag}.rvar.{Cc}", (Cc,), 0.5, 2.0)).to(dev)
        self.rep = rep

    def bn5(self, train):
        arr = (C.c_void_p * 5)()
        for i, t in enumerate([self.stats if train else None, self.gamma, self.beta, self.rmean, self.rvar]):
            arr[i] = t.data_ptr() if t is not None else None
        return arr


def _run(lib, h, dev, a, r, res, M, Mpad, Cc, relu, train, form):
    rows = GUARD_ROWS + Mpad + GUARD_ROWS
    buf = torch.full((rows, Cc), CANARY, dtype=torch.int16, device=dev)
    out = buf[GUARD_ROWS:GUARD_ROWS + Mpad]
    fin = torch.full((2, 2 * a.cpad), -7.0, dtype=torch.float32, device=dev)
    rc = lib.neraf_debug_bn_apply(h, a.x.data_ptr(), a.bn5(train), a.rep, r.x.data_ptr() if r else None, r.bn5(train) if r else None,
                                  r.rep if r else 0, res.data_ptr() if res is not None else None, M, Mpad, Cc, relu,
                                  fin[0].data_ptr(), fin[1].data_ptr(), out.data_ptr(), form, _stream())
    assert rc == 0, f"neraf_debug_bn_apply form {form} failed ({rc}): {lib.neraf_last_error(h)}"
    torch.cuda.synchronize()
    return buf.cpu().numpy(), fin.cpu().numpy()


@pytest.mark.parametrize("Cc", [64, 128, 256, 512])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 1000])
def test_tile_form_equals_small_form_bit_for_bit(lib_h, dev, M, Cc):
    lib, h = lib_h
    Mpad = (M + 127) // 128 * 128
    a = Operand("a", M, Cc, REP[M], dev)
    r = Operand("r", M, Cc, max(1, REP[M] // 2), dev)
    res = torch.from_numpy(synth.uniform(f"bn_forms.res.{M}.{Cc}", (M, Cc), -2.0, 2.0).astype(np.float16)).to(dev)
    for second, relu, train in itertools.product(("none", "residual", "bn"), (1, 0), (True, False)):
        what = f"M={M} C={Cc} second={second} relu={relu} train={train}"
        args = (a, r if second == "bn" else None, res if second == "residual" else None, M, Mpad, Cc, relu, train)
        small, fin_small = _run(lib, h, dev, *args, 0)
        tile, fin_tile = _run(lib, h, dev, *args, 1)
        for name, buf in (("small", small), ("tile", tile)):
            assert (buf[:GUARD_ROWS] == CANARY).all(), f"{what}: the {name} form wrote in front of row 0"
            assert (buf[GUARD_ROWS + Mpad:] == CANARY).all(), f"{what}: the {name} form wrote at or beyond row Mpad"
            assert (buf[GUARD_ROWS + M:GUARD_ROWS + Mpad] == 0).all(), f"{what}: rows [M, Mpad) of the {name} form are not zero"
            assert not (buf[GUARD_ROWS:GUARD_ROWS + M] == CANARY).any(), f"{what}: the {name} form left result rows unwritten"
        assert np.array_equal(small, tile), f"{what}: {int((small != tile).sum())} activations differ between the forms"
        assert np.array_equal(fin_small.view(np.uint32), fin_tile.view(np.uint32)), f"{what}: published statistics differ"
        if train:       # the pass publishes mean / biased variance of every real channel, and of nothing else
            assert (fin_tile[0, :Cc] != -7.0).all() and (fin_tile[0, a.cpad:a.cpad + Cc] != -7.0).all(), what
            assert (fin_tile[0, Cc:a.cpad] == -7.0).all(), what
            assert ((fin_tile[1, :Cc] != -7.0).all()) == (second == "bn"), what
        else:
            assert (fin_tile == -7.0).all(), what
        if relu:
            assert (tile[GUARD_ROWS:GUARD_ROWS + M].view(np.float16) >= 0).all(), what


def test_tile_form_refuses_shapes_it_cannot_cover(lib_h, dev):
    lib, h = lib_h
    a = Operand("a", 64, 72, 1, dev)          # C = 72 is no multiple of 64: only the small-launch form takes it
    out = torch.zeros((128, 72), dtype=torch.float16, device=dev)
    rc = lib.neraf_debug_bn_apply(h, a.x.data_ptr(), a.bn5(False), 1, None, None, 0, None, 64, 128, 72, 1, None, None, out.data_ptr(), 1,
                                  _stream())
    assert rc != 0
    rc = lib.neraf_debug_bn_apply(h, a.x.data_ptr(), a.bn5(False), 1, None, None, 0, None, 64, 128, 72, 1, None, None, out.data_ptr(), 0,
                                  _stream())
    torch.cuda.synchronize()
    assert rc == 0
