"""GPU tests of the streaming NT GEMM body at the two shapes whose B does not fit one workgroup's LDS and runs as two column slices
of 32 KiB each: N x K = 128 x 256 (two slices of 64 columns) and 256 x 128 (two slices of 128 columns), reached through
``neraf_gemm_f16_stream`` with body = 1, against the tile bodies of the same build (body = 2).

M in {64, 128, 192, 1000 (Mpad 1024)}, with and without add16, with and without statistics.  C16 must be bit-equal between the bodies
(same MFMA, same K order, one accumulator per element); guard rows behind Mpad keep their pattern and rows [M, Mpad) are zero.  The
atomically summed statistics are held to the bound of tests/test_gpu_gemm_stream.py, (K + M) 2^-24 sum |terms| per column against the
float64 sum of the float64 results.  Deterministic slot sums must be bit-identical between two runs and add up within the same bound.
Operands: ``neraf_amd.synth`` uniforms in [-1, 1] rounded to fp16."""
import ctypes as C

import numpy as np
import pytest
import torch

from neraf_amd import synth

pytestmark = pytest.mark.gpu

GUARD_ROWS = 64
CANARY = 0x7BCD
STRIDE = 1024
NSLOT = 40                            # >= Mpad / 32 + 2 slots / replicas allocated
PAIRS = [(128, 256), (256, 128)]
MS = [(64, 64), (128, 128), (192, 192), (1000, 1024)]


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


_HOST = {}


def _host(N, K):
    """fp16 operands for 1024 rows and their float64 products, computed once and shared (never modified)."""
    if (N, K) not in _HOST:
        a = synth.uniform(f"gemm_sliced.a.{K}", (1024, K), -1.0, 1.0).astype(np.float16)
        b = synth.uniform(f"gemm_sliced.b.{N}.{K}", (N, K), -1.0, 1.0).astype(np.float16)
        d = synth.uniform(f"gemm_sliced.add.{N}", (1024, N), -1.0, 1.0).astype(np.float16)
        _HOST[(N, K)] = dict(a=a, b=b, d=d, ab=a.astype(np.float64) @ b.astype(np.float64).T)
    return _HOST[(N, K)]


def _run(lib_h, dev, M, Mpad, N, K, body, add, stats):
    """stats: None | 'rep' (atomics into one replica) | 'det' (slot stores).  Returns (C16 bits with guard rows, sum, sumsq)."""
    lib, h = lib_h
    hst = _host(N, K)
    nan16 = np.float16(np.nan)
    A = np.full((Mpad + GUARD_ROWS, K), nan16, np.float16)
    A[:M] = hst["a"][:M]
    D = np.full((Mpad + GUARD_ROWS, N), nan16, np.float16)
    D[:M] = hst["d"][:M]
    Ad, Dd = torch.from_numpy(A.view(np.int16)).to(dev), torch.from_numpy(D.view(np.int16)).to(dev)
    Bd = torch.from_numpy(hst["b"].view(np.int16)).to(dev)
    Cd = torch.full((Mpad + GUARD_ROWS, N), CANARY, dtype=torch.int16, device=dev)
    s = torch.zeros(NSLOT, STRIDE, dtype=torch.float32, device=dev)
    q = torch.zeros(NSLOT, STRIDE, dtype=torch.float32, device=dev)
    rc = lib.neraf_gemm_f16_stream(h, Ad.data_ptr(), K, Bd.data_ptr(), K, M, N, K, Mpad, N, 1.0, None, Dd.data_ptr() if add else None, N,
                                   Cd.data_ptr(), N, None, 0, None, 0, s.data_ptr() if stats else None, q.data_ptr() if stats else None,
                                   1 if stats == "rep" else 0, STRIDE, 1 if stats == "det" else 0, body, 0, _stream())
    torch.cuda.synchronize()
    assert rc == 0, f"neraf_gemm_f16_stream body {body} N{N} K{K} M{M}: {rc} {lib.neraf_last_error(h)}"
    return Cd.cpu().numpy(), s.cpu().numpy(), q.cpu().numpy()


def _check_stats(tag, hst, M, K, add, s_sum, s_sq, N):
    ref = hst["ab"][:M] + (hst["d"][:M].astype(np.float64) if add else 0.0)
    f = (K + M) * 2.0 ** -24
    for nm, got, terms in (("sum", s_sum, ref), ("sumsq", s_sq, ref * ref)):
        want, bound = terms.sum(0), f * np.abs(terms).sum(0)
        err = np.abs(got[:N].astype(np.float64) - want)
        print(f"{tag} {nm}: max err/bound {float((err / bound).max()):.4f}")
        assert np.all(err <= bound), f"{tag} {nm}"


@pytest.mark.parametrize("M,Mpad", MS)
@pytest.mark.parametrize("N,K", PAIRS)
def test_sliced_shapes_equal_tile_bodies(lib_h, dev, N, K, M, Mpad):
    hst = _host(N, K)
    for add in (False, True):
        for stats in (None, "rep"):
            tag = f"N{N} K{K} M{M} add{int(add)} stats={stats}"
            c1, s1, q1 = _run(lib_h, dev, M, Mpad, N, K, 1, add, stats)
            c2, _, _ = _run(lib_h, dev, M, Mpad, N, K, 2, add, stats)
            assert np.array_equal(c1, c2), f"{tag}: {int((c1 != c2).sum())} elements of C16 differ between the bodies"
            assert np.all(c1[Mpad:] == CANARY), f"{tag}: rows behind Mpad written"
            assert np.all(c1[M:Mpad] == 0), f"{tag}: rows in [M, Mpad) are not zero"
            assert not np.any(c1[:M] == CANARY), f"{tag}: result rows left unwritten"
            if stats:
                assert np.all(s1[1:] == 0) and np.all(q1[1:] == 0) and np.all(s1[:, N:] == 0) and np.all(q1[:, N:] == 0), tag
                _check_stats(tag, hst, M, K, add, s1[0], q1[0], N)
            else:
                assert np.all(s1 == 0) and np.all(q1 == 0), tag


@pytest.mark.parametrize("N,K", PAIRS)
def test_sliced_deterministic_slots_reproducible(lib_h, dev, N, K):
    M, Mpad = 1000, 1024
    (c1, s1, q1), (c2, s2, q2) = [_run(lib_h, dev, M, Mpad, N, K, 1, False, "det") for _ in range(2)]
    assert np.array_equal(c1, c2) and np.array_equal(s1, s2) and np.array_equal(q1, q2)
    assert np.all(s1[:, N:] == 0) and np.all(q1[:, N:] == 0)
    tot_s, tot_q = np.zeros(STRIDE, np.float32), np.zeros(STRIDE, np.float32)
    for i in range(NSLOT):                                  # fixed order, fp32, as the consumer adds them
        tot_s += s1[i]
        tot_q += q1[i]
    _check_stats(f"det N{N} K{K}", _host(N, K), M, K, False, tot_s, tot_q, N)
