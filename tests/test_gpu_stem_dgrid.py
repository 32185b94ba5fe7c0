"""GPU test of the stem's grid gradient for a window of cells (``neraf_debug_stem_dgrid``: ``stem_dgrid_kernel``, one wave per cell,
the 27 tap slots of the cell's parity class walked without a branch) against torch's ``conv_transpose3d`` on the CPU in float64.

S = 16 (the gradient dy lives on 8^3 voxels).  Integer case: dy and the fp32 weights are integers in {-1, 0, 1} and inv_scale = 2^-3:
a cell's channel is a sum of at most 27 reaching taps x 64 output channels = 1728 integer terms, exact in fp32 (< 2^24) whatever the
order, and the scaling is exact: the result must EQUAL the reference (whose maximum before scaling is 89; asserted < 2048 below).  The windows
cover one cell, a few cells of the first row (faces and a corner of the grid), seven cells crossing a z-plane, the last 64 cells
(ending at the grid's last cell) and the whole grid -- every parity class and every face, edge and corner; n_ch = 4 and 7.  The
result buffer is longer than the window and pre-filled: nothing past [n_ch][n_cells] may be written.

Real-valued case: dy uniform in (-1, 1) rounded to fp16, weights uniform fp32.  The kernel adds at most 1728 products per lane-and-
shuffle chain in fp32, so |got - ref64| <= 1728 * 2^-24 * sum |dy w| per element (times inv_scale)."""
import ctypes as C

import numpy as np
import pytest
import torch

from neraf_amd import synth

pytestmark = pytest.mark.gpu

S = 16
SENTINEL = -12345.0
WINDOWS = [(0, 1), (0, 5), (S * S - 3, 7), (S ** 3 - 64, 64), (0, S ** 3)]


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


def _tconv(dy, w):
    """dy [d][d][d][64], w [64][7][5][5][5] (float64) -> [7][S^3]"""
    t = torch.nn.functional.conv_transpose3d(torch.from_numpy(dy).permute(3, 0, 1, 2)[None], torch.from_numpy(w), stride=2, padding=2,
                                             output_padding=1)[0]
    return t.reshape(7, -1).numpy()


_HOST = {}


def _host(kind):
    """Operands and the float64 reference over the whole grid, computed once and never modified."""
    if kind not in _HOST:
        d = S // 2
        if kind == "int":
            dy = (np.minimum(np.floor(synth.uniform("dgrid.dy", (d, d, d, 64), 0.0, 1.0) * 3.0), 2.0) - 1.0).astype(np.float64)
            w = (np.minimum(np.floor(synth.uniform("dgrid.w", (64, 7, 5, 5, 5), 0.0, 1.0) * 3.0), 2.0) - 1.0).astype(np.float64)
        else:
            dy = synth.uniform("dgrid.dyr", (d, d, d, 64), -1.0, 1.0).astype(np.float16).astype(np.float64)
            w = synth.uniform("dgrid.wr", (64, 7, 5, 5, 5), -1.0, 1.0).astype(np.float32).astype(np.float64)
        ref = _tconv(dy, w)
        if kind == "int":
            assert np.abs(ref).max() < 2048
        _HOST[kind] = dict(dy=dy.reshape(-1, 64).astype(np.float16), w=w.reshape(64, 7, 125).astype(np.float32), ref=ref,
                           mag=_tconv(np.abs(dy), np.abs(w)))
    return _HOST[kind]


def _run(lib, h, dev, ref, start, n, n_ch, inv_scale):
    dyd = torch.from_numpy(ref["dy"]).to(dev)
    wd = torch.from_numpy(ref["w"]).to(dev)
    out = torch.full((n_ch * n + 256,), SENTINEL, dtype=torch.float32, device=dev)
    rc = lib.neraf_debug_stem_dgrid(h, S, dyd.data_ptr(), wd.data_ptr(), start, n, n_ch, inv_scale, out.data_ptr(), _stream())
    assert rc == 0, lib.neraf_last_error(h)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[n_ch * n:] == SENTINEL).all(), "written past [n_ch][n_cells]"
    return out[:n_ch * n].reshape(n_ch, n).astype(np.float64)


@pytest.mark.parametrize("n_ch", [4, 7])
@pytest.mark.parametrize("start,n", WINDOWS)
def test_grid_gradient_window_exact(lib_h, dev, start, n, n_ch):
    lib, h = lib_h
    ref = _host("int")
    got = _run(lib, h, dev, ref, start, n, n_ch, 0.125)
    want = ref["ref"][:n_ch, start:start + n] * 0.125
    bad = got != want
    assert not bad.any(), f"window ({start}, {n}) n_ch {n_ch}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0]}"


def test_grid_gradient_real_values_within_fp32_chain_bound(lib_h, dev):
    lib, h = lib_h
    ref = _host("real")
    got = _run(lib, h, dev, ref, 0, S ** 3, 7, 0.5)
    err = np.abs(got - ref["ref"] * 0.5)
    bound = 1728 * 2.0 ** -24 * ref["mag"] * 0.5
    print(f"max err {err.max():.3e}, max err / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()
