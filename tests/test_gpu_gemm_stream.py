"""GPU tests of the streaming NT GEMM body (``gemm_f16_nt_stream_kernel``, reached through ``neraf_gemm_f16_stream``): the plain
fp16 GEMMs of ResNet3D layer 1, whose whole B operand (N * K <= 16384 elements) stays in one workgroup's LDS while A is streamed in
64-row blocks.  body = 1 forces the streaming body, body = 2 the tile bodies of the same build, body = 0 is the dispatcher's choice.

Inputs are ``neraf_amd.synth`` uniforms in [-1, 1] rounded to fp16; the reference is the float64 product of those fp16 values,
times alpha, plus add16, formed on the host.  Bounds (derived, not tuned):

    * C16: |c - ref| <= 2^-11 |ref| + K 2^-24 sum_k |a b| + 2^-24 -- the fp16 rounding of the result (half an ulp is at most
      2^-11 |ref|; 2^-24 is the subnormal spacing), and K roundings of 2^-24 relative in the fp32 accumulation.  The comparison is with
      the UNROUNDED float64 reference: c is the fp16 rounding of an fp32 value a few 2^-24 away from ref, so wherever ref lies that
      close to the midpoint of two fp16 numbers c may be either of them -- a whole fp16 ulp from "ref rounded to fp16", which no
      implementation with fp32 accumulators can avoid (the tile bodies do the same; the count is printed).  Every c that equals the
      rounded reference passes this comparison, so it asks nothing less of an exact result.
    * a statistic: |s - sum64| <= (K + M) 2^-24 sum |terms| of its column (terms: the float64 results, or their squares).
    * C16 is bit-equal to the tile bodies' (body = 2) on the same operands: same MFMA, same K order, one accumulator per element.

Shapes are the smallest that still exercise the walk: M = 4096 is 64 row blocks of 64 rows.  A workgroup is two walkers of four waves
and holds at most 128 columns (N = 256 runs as two column slices per row group), so max_workgroups = 3 leaves one row group at
N = 256 (two walkers of 32 blocks) and three at N = 64 (six walkers of 10 or 11 blocks): the prefetch of the next block and the sums
carried across blocks are exercised."""
import ctypes as C

import numpy as np
import pytest
import torch

from neraf_amd import synth

pytestmark = pytest.mark.gpu

EINVAL = -1
GUARD_ROWS = 64
CANARY = 0x7BCD                      # fp16 bit pattern of 63904: no result of these inputs (|c| <= K + 1) has it
STRIDE = 1024                        # floats between statistic replicas / slots
NREP_ALLOC = 32                      # replicas allocated; at most 16 may be touched
PAIRS = [(64, 64), (64, 128), (64, 256), (128, 64), (128, 128), (256, 64)]     # every (N, K) of the body: N * K <= 16384


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


def _host(M, N, K):
    """fp16 operands and float64 references of one shape, computed once and shared (never modified)."""
    key = (M, N, K)
    if key not in _HOST:
        a = synth.uniform(f"gemm_stream.a.{M}.{K}", (M, K), -1.0, 1.0).astype(np.float16)
        b = synth.uniform(f"gemm_stream.b.{N}.{K}", (N, K), -1.0, 1.0).astype(np.float16)
        d = synth.uniform(f"gemm_stream.add.{M}.{N}", (M, N), -1.0, 1.0).astype(np.float16)
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        _HOST[key] = dict(a=a, b=b, d=d, ab=a64 @ b64.T, absab=np.abs(a64) @ np.abs(b64).T)
    return _HOST[key]


class Run:
    """One launch: device buffers with canaries / guards, the call, and the results back on the host."""

    def __init__(self, lib_h, dev, M, N, K, *, Mpad=None, body=1, max_wg=0, alpha=1.0, add=False, pad_ld=0, stats=None, stat_rep=1,
                 host=None):
        lib, h = lib_h
        Mpad = Mpad or M
        hst = host or _host(M, N, K)
        lda, ldc, ldadd = K + pad_ld, N + pad_ld, N + pad_ld
        rows = Mpad + GUARD_ROWS
        nan16 = np.float16(np.nan)
        A = np.full((rows, lda), nan16, np.float16)          # pad rows, pad columns and the guard hold NaN: whatever reads them shows
        A[:M, :K] = hst["a"][:M]
        D = np.full((rows, ldadd), nan16, np.float16)
        D[:M, :N] = hst["d"][:M]
        self.A0, self.D0 = A, D
        self.A = torch.from_numpy(A.view(np.int16)).to(dev)
        self.D = torch.from_numpy(D.view(np.int16)).to(dev) if add else None
        self.B = torch.from_numpy(hst["b"].view(np.int16)).to(dev)
        self.Cdev = torch.full((rows, ldc), CANARY, dtype=torch.int16, device=dev)
        self.sum = self.sq = None
        nslots = max(NREP_ALLOC, Mpad // 32 + 2)
        if stats:
            self.sum = torch.zeros(nslots, STRIDE, dtype=torch.float32, device=dev)
            self.sq = torch.zeros(nslots, STRIDE, dtype=torch.float32, device=dev)
        self.M, self.N, self.K, self.Mpad, self.alpha, self.add = M, N, K, Mpad, alpha, add
        self.rc = lib.neraf_gemm_f16_stream(
            h, self.A.data_ptr(), lda, self.B.data_ptr(), K, M, N, K, Mpad, N, alpha, None,
            self.D.data_ptr() if add else None, ldadd, self.Cdev.data_ptr(), ldc, None, 0, None, 0,
            self.sum.data_ptr() if stats else None, self.sq.data_ptr() if stats else None,
            stat_rep if stats == "rep" else 0, STRIDE, 1 if stats == "det" else 0, body, max_wg, _stream())
        torch.cuda.synchronize()
        self.Cbits = self.Cdev.cpu().numpy()
        self.host = hst

    def ref(self):
        r = self.alpha * self.host["ab"][:self.M]
        if self.add:
            r = r + self.host["d"][:self.M].astype(np.float64)
        return r

    def c16(self):
        return self.Cbits[:self.M, :self.N].view(np.float16)

    def check_c16(self, tag):
        ref, c = self.ref(), self.c16().astype(np.float64)
        bound = 2.0 ** -11 * np.abs(ref) + self.K * 2.0 ** -24 * self.host["absab"][:self.M] + 2.0 ** -24
        err = np.abs(c - ref)
        with np.errstate(over="ignore"):
            off = int((self.c16() != ref.astype(np.float16)).sum())
        print(f"{tag}: max err/bound {float((err / bound).max()):.3f}; {off} of {ref.size} elements are not the rounded reference")
        assert np.all(np.isfinite(c)) and np.all(err <= bound), tag

    def check_guards(self, tag):
        assert np.all(self.Cbits[:, self.N:] == CANARY), f"{tag}: pad columns of C16 written"
        assert np.all(self.Cbits[self.Mpad:] == CANARY), f"{tag}: rows behind Mpad of C16 written"
        assert np.all(self.Cbits[self.M:self.Mpad, :self.N] == 0), f"{tag}: rows in [M, Mpad) of C16 are not zero"
        assert np.array_equal(self.A.cpu().numpy(), self.A0.view(np.int16)), f"{tag}: A changed"
        if self.add:
            assert np.array_equal(self.D.cpu().numpy(), self.D0.view(np.int16)), f"{tag}: add16 changed"

    def check_stats(self, tag, s_sum, s_sq):
        ref = self.ref()
        f = (self.K + self.M) * 2.0 ** -24
        for nm, got, terms in (("sum", s_sum, ref), ("sumsq", s_sq, ref * ref)):
            want, bound = terms.sum(0), f * np.abs(terms).sum(0)
            err = np.abs(got[:self.N].astype(np.float64) - want)
            print(f"{tag} {nm}: max err/bound {float((err / bound).max()):.4f}")
            assert np.all(err <= bound), f"{tag} {nm}"


def _same_bits(r1, r2, tag):
    assert r1.rc == 0 and r2.rc == 0, tag
    assert np.array_equal(r1.Cbits, r2.Cbits), f"{tag}: C16 differs between the bodies"


@pytest.mark.parametrize("N,K", PAIRS)
def test_basic_shapes(lib_h, dev, N, K):
    """1. every (N, K) of the body at M = Mpad = 4096, one row block per workgroup: within the bounds, bit-equal to the tile bodies."""
    r1 = Run(lib_h, dev, 4096, N, K, body=1, stats="rep", stat_rep=1)
    r2 = Run(lib_h, dev, 4096, N, K, body=2)
    assert r1.rc == 0
    r1.check_c16(f"N{N} K{K}")
    r1.check_guards(f"N{N} K{K}")
    r1.check_stats(f"N{N} K{K}", r1.sum[0].cpu().numpy(), r1.sq[0].cpu().numpy())
    _same_bits(r1, r2, f"N{N} K{K}")


@pytest.mark.parametrize("N,K,max_wg", [(256, 64, 3), (64, 256, 3), (256, 64, 6)])
def test_loop_carry(lib_h, dev, N, K, max_wg):
    """2. at most three workgroups walk the 64 row blocks (N = 256: one row group in two column slices, two walkers of 32 blocks;
    N = 64: three row groups, six walkers of 10 or 11 blocks; the third case, six workgroups at N = 256, has the uneven walks there):
    the next block's prefetch and the sums carried across blocks."""
    r1 = Run(lib_h, dev, 4096, N, K, body=1, max_wg=max_wg, stats="rep", stat_rep=1)
    r2 = Run(lib_h, dev, 4096, N, K, body=2)
    assert r1.rc == 0
    r1.check_c16(f"carry N{N} K{K}")
    r1.check_guards(f"carry N{N} K{K}")
    r1.check_stats(f"carry N{N} K{K}", r1.sum[0].cpu().numpy(), r1.sq[0].cpu().numpy())
    _same_bits(r1, r2, f"carry N{N} K{K}")


@pytest.mark.parametrize("N,K,max_wg", [(256, 64, 0), (64, 256, 5), (128, 128, 0)])
def test_ragged_m(lib_h, dev, N, K, max_wg):
    """3. M = 4000 in Mpad = 4032 with lda = K + 8, ldc16 = ldadd = N + 8: rows 4000..4031 are zeros (their A and add16 rows hold NaN),
    the pad columns and the 64 guard rows behind Mpad of every buffer keep their pattern, the statistics ignore the pad rows."""
    tag = f"ragged N{N} K{K}"
    host = _host(4096, N, K)
    r1 = Run(lib_h, dev, 4000, N, K, Mpad=4032, body=1, max_wg=max_wg, add=True, pad_ld=8, stats="rep", stat_rep=1, host=host)
    r2 = Run(lib_h, dev, 4000, N, K, Mpad=4032, body=2, add=True, pad_ld=8, host=host)
    assert r1.rc == 0
    r1.check_c16(tag)
    r1.check_guards(tag)
    r1.check_stats(tag, r1.sum[0].cpu().numpy(), r1.sq[0].cpu().numpy())
    _same_bits(r1, r2, tag)


@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("alpha", [1.0, 0.5])
def test_add16_and_alpha(lib_h, dev, add, alpha):
    """4. add16 present and absent, alpha 1 and 0.5 (N, K = 256, 64, the dgrad shape that carries add16 in layer 1)."""
    tag = f"add{int(add)} alpha{alpha}"
    r1 = Run(lib_h, dev, 4096, 256, 64, body=1, max_wg=7, alpha=alpha, add=add)
    r2 = Run(lib_h, dev, 4096, 256, 64, body=2, alpha=alpha, add=add)
    assert r1.rc == 0
    r1.check_c16(tag)
    r1.check_guards(tag)
    _same_bits(r1, r2, tag)


@pytest.mark.parametrize("N,K", [(256, 64), (64, 256)])
@pytest.mark.parametrize("rep", [1, 16])
def test_statistics_replicas(lib_h, dev, N, K, rep):
    """5a. atomic statistics: the sum over the stat_rep replicas is within the bound; no replica at or beyond stat_rep and no column
    at or beyond N is touched."""
    r = Run(lib_h, dev, 4096, N, K, body=1, max_wg=40, stats="rep", stat_rep=rep)
    assert r.rc == 0
    s, q = r.sum.cpu().numpy(), r.sq.cpu().numpy()
    for buf in (s, q):
        assert np.all(buf[rep:] == 0) and np.all(buf[:, N:] == 0)
    if rep > 1:
        assert np.count_nonzero(np.abs(s[:rep]).sum(1)) == rep          # 20 or more row groups spread over all 16 replicas
    r.check_stats(f"rep{rep} N{N} K{K}", s[:rep].sum(0, dtype=np.float64), q[:rep].sum(0, dtype=np.float64))


@pytest.mark.parametrize("N,K,max_wg", [(256, 64, 0), (64, 256, 3)])
def test_statistics_deterministic(lib_h, dev, N, K, max_wg):
    """5b. stat_det: slot = first row / 32 of the workgroup's first block holds its sums (a plain store), every other slot keeps the
    caller's zero; the slots added in order are within the bound; two runs are bit-identical.  Row group rg (all column slices of
    it) starts at block 2 rg, row 128 rg: slot 4 rg; 64 blocks make at most 32 row groups (fewer CUs than 64 would make fewer)."""
    runs = [Run(lib_h, dev, 4096, N, K, body=1, max_wg=max_wg, stats="det") for _ in range(2)]
    assert all(r.rc == 0 for r in runs)
    s, q = runs[0].sum.cpu().numpy(), runs[0].sq.cpu().numpy()
    assert np.array_equal(s, runs[1].sum.cpu().numpy()) and np.array_equal(q, runs[1].sq.cpu().numpy())
    slices = N // 128 if N > 128 else 1
    nrg = min(max_wg // slices, 32) if max_wg else 32
    owned = np.zeros(s.shape[0], bool)
    owned[4 * np.arange(nrg)] = True
    for buf in (s, q):
        assert np.all(buf[~owned] == 0) and np.all(buf[:, N:] == 0)
        assert np.all(np.abs(buf[owned][:, :N]).sum(1) > 0)
    tot_s, tot_q = np.zeros(STRIDE, np.float32), np.zeros(STRIDE, np.float32)
    for i in range(s.shape[0]):                            # fixed order, fp32, as the consumer adds them
        tot_s += s[i]
        tot_q += q[i]
    runs[0].check_stats(f"det N{N} K{K}", tot_s, tot_q)


def test_refusals(lib_h, dev):
    """6. body = 1 with bias, C16T, C32, N = 192 or K = 512 returns NERAF_EINVAL and writes nothing."""
    lib, h = lib_h
    M = 256
    A = torch.zeros(M, 512, dtype=torch.float16, device=dev)
    B = torch.zeros(256, 512, dtype=torch.float16, device=dev)
    bias = torch.zeros(256, dtype=torch.float32, device=dev)

    def call(N, K, bias_p=None, c16t=False, c32=False):
        Cd = torch.full((M, 256), CANARY, dtype=torch.int16, device=dev)
        Ct = torch.full((256, M), CANARY, dtype=torch.int16, device=dev)
        Cf = torch.full((M, 256), 7.0, dtype=torch.float32, device=dev)
        rc = lib.neraf_gemm_f16_stream(h, A.data_ptr(), 512, B.data_ptr(), 512, M, N, K, M, N, 1.0, bias_p, None, 0, Cd.data_ptr(), 256,
                                       Ct.data_ptr() if c16t else None, M, Cf.data_ptr() if c32 else None, 256, None, None, 0, STRIDE, 0,
                                       1, 0, _stream())
        torch.cuda.synchronize()
        untouched = bool((Cd == CANARY).all()) and bool((Ct == CANARY).all()) and bool((Cf == 7.0).all())
        return rc, untouched

    assert call(256, 64)[0] == 0                                        # the qualifying form of the same call
    for kw in (dict(N=256, K=64, bias_p=bias.data_ptr()), dict(N=256, K=64, c16t=True), dict(N=256, K=64, c32=True),
               dict(N=192, K=64), dict(N=64, K=512)):
        rc, untouched = call(**kw)
        assert rc == EINVAL and untouched, kw


def test_dispatch(lib_h, dev):
    """7. body = 0 takes the streaming body at (32768, 256, 64) -- same bits as body = 1 -- and leaves (4096, 512, 128) and
    (512, 1024, 256), shapes of the 4096- and 512-voxel layers, on the tile bodies -- same bits as body = 2."""
    lib, h = lib_h

    def bits(M, N, K, body):
        a = torch.from_numpy(synth.uniform(f"gemm_stream.da.{M}.{K}", (M, K), -1.0, 1.0).astype(np.float16).view(np.int16)).to(dev)
        b = torch.from_numpy(synth.uniform(f"gemm_stream.db.{N}.{K}", (N, K), -1.0, 1.0).astype(np.float16).view(np.int16)).to(dev)
        c = torch.full((M, N), CANARY, dtype=torch.int16, device=dev)
        rc = lib.neraf_gemm_f16_stream(h, a.data_ptr(), K, b.data_ptr(), K, M, N, K, M, N, 1.0, None, None, 0, c.data_ptr(), N, None, 0,
                                       None, 0, None, None, 0, STRIDE, 0, body, 0, _stream())
        torch.cuda.synchronize()
        assert rc == 0, (M, N, K, body)
        return c.cpu().numpy()

    c0, c1 = bits(32768, 256, 64, 0), bits(32768, 256, 64, 1)
    assert np.array_equal(c0, c1) and not np.any(c0 == CANARY)
    for M, N, K in ((4096, 512, 128), (512, 1024, 256)):
        c0, c2 = bits(M, N, K, 0), bits(M, N, K, 2)
        assert np.array_equal(c0, c2) and not np.any(c0 == CANARY)


def test_dispatch_keeps_deterministic_statistics(lib_h, dev):
    """7b. with stat_det the dispatcher (body = 0) stays on the tile body where statistics are asked for: at (32768, 256, 64) every slot
    and C16 have the bits of body = 2, so a deterministic run computes what it computed before the streaming body existed; without
    statistics the same call streams (test_dispatch).  body = 1 fills other slots (one per row group, test_statistics_deterministic)."""
    M, N, K = 32768, 256, 64
    runs = {body: Run(lib_h, dev, M, N, K, body=body, stats="det", host=_host(M, N, K)) for body in (0, 2, 1)}
    assert all(r.rc == 0 for r in runs.values())
    s = {b: r.sum.cpu().numpy() for b, r in runs.items()}
    q = {b: r.sq.cpu().numpy() for b, r in runs.items()}
    assert np.array_equal(s[0], s[2]) and np.array_equal(q[0], q[2]) and np.array_equal(runs[0].Cbits, runs[2].Cbits)
    assert np.array_equal(runs[0].Cbits, runs[1].Cbits)
    assert not np.array_equal(s[0] != 0, s[1] != 0)          # the forced streaming body owns other slots: it was not what body 0 ran
