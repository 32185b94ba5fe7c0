"""GPU tests of the stride-2 transposed-convolution launches alone (``neraf_debug_conv_transpose``) against torch's
``conv_transpose3d`` on the CPU in float64: the 1x1x1 residual-branch dgrad -- added in place it is ONE plain GEMM over the reaching
parity class (row r of the source lands on voxel (2z, 2y, 2x)), otherwise the eight-class launch -- and the 3x3x3 parity-class dgrad,
whose tiles every XCD walks heaviest class first where 64 divides the number of row tiles (din = 16 on 32-row tiles, din = 32 on
64-row tiles: launches of more than 256 tiles of 64x64 keep that shape) and in alternating order elsewhere (din = 8).

dy and w are integers in {-1, 0, 1} and the destination's previous content (add16) integers in -8 .. 8: an element is a sum of at most
1024 (1x1x1, cout = 1024) or 8 taps x 256 (3x3x3) terms plus add16, exact in the fp32 accumulators and -- while |.| <= 2048 -- in fp16,
whatever the summation order: the result must EQUAL the reference.  The reference's maximum is asserted per case (the largest over
all cases here is 115, 121 with add16).  `din` is the edge of the RESULT (the convolution's input); the source has (din / 2)^3 voxels.

1x1x1, in place: the seven classes no tap reaches must keep their bits (checked bit for bit against a copy), canary rows around
the buffer stay intact, and the launch record names the body: the 32x32 tile form up to 128 tiles of 64x64 (every size but
din = 32, which is the layer-2 launch of the encoder itself: 256 tiles, 64x64 form)."""
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


def _ints(tag, shape, lo, hi):
    return np.minimum(np.floor(synth.uniform(tag, shape, 0.0, 1.0) * (hi - lo + 1)) + lo, hi).astype(np.float64)


_HOST = {}


def _host(cin, cout, k, din):
    """Integer operands, the previous destination content and the float64 transposed convolution: once per case, never modified."""
    key = (cin, cout, k, din)
    if key not in _HOST:
        d = din // 2
        tag = f"tconv.{cin}.{cout}.{k}.{din}"
        dy = _ints(tag + ".dy", (d, d, d, cout), -1, 1)
        w = _ints(tag + ".w", (cout, cin, k, k, k), -1, 1)
        add = _ints(tag + ".add", (din ** 3, cin), -8, 8)
        t = torch.nn.functional.conv_transpose3d(torch.from_numpy(dy).permute(3, 0, 1, 2)[None], torch.from_numpy(w), stride=2,
                                                 padding=k // 2, output_padding=1)[0]          # [cin][din]^3, float64
        ref = t.permute(1, 2, 3, 0).reshape(din ** 3, cin).numpy()
        assert np.abs(ref).max() + 8 <= 2048
        z, y, x = np.meshgrid(np.arange(din), np.arange(din), np.arange(din), indexing="ij")
        even = ((z | y | x) & 1).reshape(-1) == 0
        _HOST[key] = dict(dy=dy.reshape(-1, cout).astype(np.float16), w=w.reshape(cout, cin, k ** 3).astype(np.float32),
                          add=add.astype(np.float16), ref=ref, even=even)
    return _HOST[key]


def _run(lib, h, dev, cin, cout, k, din, dst16, in_place, manifest=False):
    """dst16: fp16 [din^3][cin] previous content of the destination.  Returns the destination afterwards (fp16) and the launch records."""
    ref = _host(cin, cout, k, din)
    M = din ** 3
    dyd = torch.from_numpy(ref["dy"]).to(dev)
    wd = torch.from_numpy(ref["w"]).to(dev)
    buf = torch.full((GUARD_ROWS + M + GUARD_ROWS, cin), CANARY, dtype=torch.int16, device=dev)
    buf[GUARD_ROWS:GUARD_ROWS + M] = torch.from_numpy(dst16.view(np.int16)).to(dev)
    names = []
    if manifest:
        lib.neraf_manifest_enable(h, 1)
    try:
        rc = lib.neraf_debug_conv_transpose(h, cin, cout, k, din, dyd.data_ptr(), wd.data_ptr(), buf[GUARD_ROWS:].data_ptr(), in_place, _stream())
        assert rc == 0, lib.neraf_last_error(h)
        torch.cuda.synchronize()
        if manifest:
            name = C.create_string_buffer(160)
            for i in range(lib.neraf_manifest_get(h, -1, None, 0, None, None, None)):
                lib.neraf_manifest_get(h, i, name, 160, None, None, None)
                names.append(name.value.decode())
    finally:
        if manifest:
            lib.neraf_manifest_enable(h, 0)
    out = buf.cpu().numpy()
    assert (out[:GUARD_ROWS] == CANARY).all() and (out[GUARD_ROWS + M:] == CANARY).all(), "written outside the destination"
    return out[GUARD_ROWS:GUARD_ROWS + M].view(np.float16), names


def _assert_equal(got16, want, what):
    bad = got16.astype(np.float64) != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at row/col {np.argwhere(bad)[0]}"


K1_CASES = [(256, 512, 8), (256, 512, 16), (512, 1024, 8), (512, 1024, 16), (256, 512, 32)]


@pytest.mark.parametrize("cin,cout,din", K1_CASES)
def test_strided_1x1x1_in_place_is_one_compact_launch(lib_h, dev, cin, cout, din):
    lib, h = lib_h
    ref = _host(cin, cout, 1, din)
    got, names = _run(lib, h, dev, cin, cout, 1, din, ref["add"], 1, manifest=True)
    _assert_equal(got, ref["ref"] + ref["add"].astype(np.float64), f"1x1x1 {cin}<-{cout} din {din} in place")
    odd = ~ref["even"]
    assert (got.view(np.int16)[odd] == ref["add"].view(np.int16)[odd]).all(), "a class no tap reaches lost its bits"
    rows, tiles = (din // 2) ** 3, ((din // 2) ** 3 // 64) * (cin // 64)
    body = "<32, 32" if tiles <= 128 else "<64, 64"
    gemms = [n for n in names if n.startswith("gemm_f16_nt_")]
    assert len(gemms) == 1 and gemms[0].startswith(f"gemm_f16_nt_pipe_kernel{body} | dgrad s2 compact M={rows} N={cin} K={cout}"), names


@pytest.mark.parametrize("cin,cout,din", K1_CASES[:4])
def test_strided_1x1x1_zeroed_and_overwritten_destination(lib_h, dev, cin, cout, din):
    lib, h = lib_h
    ref = _host(cin, cout, 1, din)
    zero = np.zeros((din ** 3, cin), np.float16)
    got, _ = _run(lib, h, dev, cin, cout, 1, din, zero, 1)
    _assert_equal(got, ref["ref"], "in place on zeros")
    assert (got.view(np.int16)[~ref["even"]] == 0).all()
    got, names = _run(lib, h, dev, cin, cout, 1, din, ref["add"], 0, manifest=True)      # eight classes: all of dx is rewritten
    _assert_equal(got, ref["ref"], "overwrite")
    assert not any("compact" in n for n in names), names


@pytest.mark.parametrize("cin,cout,din", [(128, 128, 8), (128, 128, 16), (256, 256, 8), (64, 64, 32)])
@pytest.mark.parametrize("in_place", [0, 1])
def test_strided_3x3x3_every_class_exact(lib_h, dev, cin, cout, din, in_place):
    lib, h = lib_h
    ref = _host(cin, cout, 3, din)
    got, names = _run(lib, h, dev, cin, cout, 3, din, ref["add"], in_place, manifest=True)
    want = ref["ref"] + (ref["add"].astype(np.float64) if in_place else 0.0)
    _assert_equal(got, want, f"3x3x3 {cin}<-{cout} din {din} in_place {in_place}")
    tiles = (din ** 3 // 64) * (cin // 64)
    body = "<32, 32" if tiles <= 256 else "<64, 64"          # 32-row tiles while all of them are resident at once
    gemms = [n for n in names if n.startswith("gemm_f16_nt_")]
    assert len(gemms) == 1 and gemms[0].startswith(f"gemm_f16_nt_pipe_kernel{body} | dgrad M={din ** 3} N={cin} K={27 * cout}"), names
