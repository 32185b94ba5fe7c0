"""GPU tests of the grouped fp16 GEMM launch (``neraf_gemm_f16_grouped``: up to six plain GEMMs of any shapes that share K, lda and ldb
in one grid) and of the NAcF backward that issues its narrow weight gradients -- heads, layers 4, 3, 2 and the query columns of layer 0 --
through it behind the dX chain (profiles/nacf_grouped_wgrad_ab.txt; the "nacf_like" case below has their shapes).

What must hold:
    * a group's result is the result of that group's own launch BIT FOR BIT: every 4-wave body adds an output element's K-steps in
      the same order with the same MFMA shape whatever the tile, and these GEMMs have no atomics;
    * on small integers (all products and sums exact in fp16 x fp16 -> fp32) it is the integer matmul;
    * the NAcF gradients stay within the tolerance of tests/test_gpu_nacf.py (same comparison, same numbers, imported from there);
    * the workspace the library asks for covers everything the backward touches, and nothing of one backward leaks into the next.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from neraf_amd import synth
from test_gpu_nacf import GRAD_REL_L2, OUT_MAX_ABS, OUT_REL_L2, T, _make_field, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _up(x, m):
    return (x + m - 1) // m * m


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


GUARD = 64          # floats behind every result, which no launch may touch


def _grouped(lib, h, As, Bs, Ms, Ns, Cs, K, alpha, alpha_dev, beta, ldcs=None, ws=None):
    from neraf_amd import _lib
    n = len(As)
    _lib.check(lib.neraf_gemm_f16_grouped(h, n, _lib.ptr_array(As), _lib.ptr_array(Bs), (C.c_int * n)(*Ms), (C.c_int * n)(*Ns),
                                          _lib.ptr_array(Cs), (C.c_int * n)(*(ldcs or Ns)), K, K, K, alpha,
                                          alpha_dev.data_ptr() if alpha_dev is not None else None, beta,
                                          ws.data_ptr() if ws is not None else None, ws.numel() * 4 if ws is not None else 0, _stream()))


# (name, [(M, N) per group], K, c32_beta, alpha, alpha_dev).  64x64 tiles of a launch = sum ceil(M/64) ceil(N/64); up to 128 of them the
# launcher takes 32x32 tiles, above 64x64.  alpha and alpha_dev are powers of two (exact on the integer inputs).
CASES = [
    ("one_group", [(513, 512)], 192, 0, 1.0, None),
    ("two_groups_ragged_one_kstep", [(130, 64), (64, 1000)], 64, 1, 1.0, None),                                   # 19 tiles
    ("six_groups_long_k", [(513, 512), (130, 64), (64, 1000), (64, 64), (200, 300), (64, 163)], 2048, 0, 0.5, 0.25),   # 115 tiles
    ("six_groups_128_tiles", [(513, 512), (64, 1000), (130, 64), (64, 64), (320, 448), (64, 64)], 192, 0, 1.0, None),
    ("six_groups_129_tiles", [(513, 512), (64, 1000), (130, 64), (64, 64), (320, 448), (64, 128)], 192, 1, 1.0, 0.25),
    ("single_tile_groups", [(64, 64), (1, 1)], 64, 0, 2.0, None),
    ("equal_shape_field_form", [(64, 32), (16, 64), (64, 64), (64, 64), (16, 64)], 2048, 1, 1.0, 0.125),
    ("nacf_like", [(513, 512), (512, 1024), (1024, 1024), (1024, 2048), (5096, 163)], 128, 0, 1.0, 0.5),          # 1208 tiles
    # results that are column blocks of wider matrices (ldc32 = N + 37, the layer-0 query columns' form): the columns between stay untouched
    ("wide_ldc", [(130, 163), (64, 64), (200, 300)], 192, 1, 1.0, 0.5),
    # with scratch: five equal-shape tiles and 32 K-steps are split along K (8 slices of 4 K-steps, as each group's own launch is)
    ("equal_shape_split_k", [(64, 32), (16, 64), (64, 64), (64, 64), (16, 64)], 2048, 1, 1.0, 0.125),
]


def test_case_list_crosses_the_tile_selector():
    tiles = {c[0]: sum(_up(m, 64) // 64 * (_up(n, 64) // 64) for m, n in c[1]) for c in CASES}
    assert tiles["six_groups_128_tiles"] == 128 and tiles["six_groups_129_tiles"] == 129
    assert {len(c[1]) for c in CASES} >= {1, 2, 6}


@pytest.mark.parametrize("kind", ["int", "random"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_grouped_equals_separate_launches(dev, case, kind):
    from neraf_amd import _lib
    lib = _lib.load()
    h = _lib.ctx(0)
    _, shapes, K, beta, alpha, adev = case
    rng = np.random.default_rng(4242 + 7 * K + len(shapes) + beta)
    As, Bs, Ms, Ns, inits, refs = [], [], [], [], [], []
    for (M, N) in shapes:
        Mp, Np = _up(M, 64), _up(N, 64)
        # the padding rows hold data too: only the M x N corner of a tile may reach the result
        if kind == "int":
            A = rng.integers(-3, 4, size=(Mp, K)).astype(np.float32)
            B = rng.integers(-2, 3, size=(Np, K)).astype(np.float32)
            init = rng.integers(-5, 6, size=(M, N)).astype(np.float32)
        else:
            A = rng.standard_normal((Mp, K)).astype(np.float32)
            B = rng.standard_normal((Np, K)).astype(np.float32)
            init = rng.standard_normal((M, N)).astype(np.float32)
        As.append(T(A, dev).half()); Bs.append(T(B, dev).half()); Ms.append(M); Ns.append(N); inits.append(init)
        if kind == "int":
            s = np.float32(alpha) * np.float32(adev if adev is not None else 1.0)
            refs.append(((A[:M].astype(np.float64) @ B[:N].astype(np.float64).T) * float(s) + (init if beta else 0.0)).astype(np.float32))
    adev_t = torch.tensor([adev], dtype=torch.float32, device=dev) if adev is not None else None
    pad = 37 if case[0] == "wide_ldc" else 0
    ldcs = [N + pad for N in Ns]

    def fresh():          # [M][ldc] + GUARD floats, 7.0 wherever no result belongs
        out = []
        for init, ldc in zip(inits, ldcs):
            M, N = init.shape
            c = torch.full((M * ldc + GUARD,), 7.0, dtype=torch.float32, device=dev)
            c[:M * ldc].view(M, ldc)[:, :N] = T(init, dev)
            out.append(c)
        return out

    ws = torch.zeros(4 << 20, dtype=torch.float32, device=dev) if case[0] == "equal_shape_split_k" else None
    Cg = fresh()
    _grouped(lib, h, As, Bs, Ms, Ns, Cg, K, alpha, adev_t, beta, ldcs, ws)
    Cs = fresh()
    for g in range(len(shapes)):          # a table of one is the ordinary single launch
        _grouped(lib, h, As[g:g + 1], Bs[g:g + 1], Ms[g:g + 1], Ns[g:g + 1], Cs[g:g + 1], K, alpha, adev_t, beta, ldcs[g:g + 1], ws)
    Cp = None
    if adev is None and beta == 0:        # neraf_gemm_f16 itself has neither a device scalar nor an accumulate flag
        Cp = fresh()
        for g, (M, N) in enumerate(shapes):
            _lib.check(lib.neraf_gemm_f16(h, As[g].data_ptr(), K, Bs[g].data_ptr(), K, M, N, K, _up(M, 64), _up(N, 64), alpha, None, 0,
                                          None, 0, None, 0, Cp[g].data_ptr(), N, _stream()))
    torch.cuda.synchronize()
    for g, (M, N) in enumerate(shapes):
        got = Cg[g].cpu().numpy()
        ldc = ldcs[g]
        assert (got[M * ldc:] == 7.0).all(), f"group {g}: wrote behind its result"
        assert (got[:M * ldc].reshape(M, ldc)[:, N:] == 7.0).all(), f"group {g}: wrote between its rows"
        np.testing.assert_array_equal(got, Cs[g].cpu().numpy(), err_msg=f"group {g} vs its own launch")
        if Cp is not None:
            np.testing.assert_array_equal(got, Cp[g].cpu().numpy(), err_msg=f"group {g} vs neraf_gemm_f16")
        if kind == "int":
            np.testing.assert_array_equal(got[:M * ldc].reshape(M, ldc)[:, :N], refs[g], err_msg=f"group {g} vs the integer matmul")


def test_grouped_rejects_bad_tables(dev):
    from neraf_amd import _lib
    lib = _lib.load()
    h = _lib.ctx(0)
    a = torch.zeros((64, 64), dtype=torch.float16, device=dev)
    c = torch.zeros((64 * 64,), dtype=torch.float32, device=dev)
    seven = [a] * 7
    rc = lib.neraf_gemm_f16_grouped(h, 7, _lib.ptr_array(seven), _lib.ptr_array(seven), (C.c_int * 7)(*[64] * 7), (C.c_int * 7)(*[64] * 7),
                                    _lib.ptr_array([c] * 7), (C.c_int * 7)(*[64] * 7), 64, 64, 64, 1.0, None, 0, None, 0, _stream())
    assert rc != 0
    rc = lib.neraf_gemm_f16_grouped(h, 2, _lib.ptr_array([a, a]), _lib.ptr_array([a, a]), (C.c_int * 2)(64, 0), (C.c_int * 2)(64, 64),
                                    _lib.ptr_array([c, c]), (C.c_int * 2)(64, 64), 64, 64, 64, 1.0, None, 0, None, 0, _stream())
    assert rc != 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,F_,T_", [(1, 513, 60), (2, 257, 101)])
@pytest.mark.parametrize("B", [1, 60, 200])
def test_nacf_backward_vs_oracle(dev, B, C_, F_, T_):
    """forward_queries + backward against the oracle: the comparison and the tolerances of
    tests/test_gpu_nacf.py::test_split_forward_backward_vs_oracle, every weight and bias gradient."""
    from oracle import audio as O
    f, sd = _make_field(C_, F_, dev)
    b = synth.audio_batch(B, C_, F_, T_, tag=f"t.grouped{B}")
    aabb = T(synth.audio_aabb())
    feat = T(synth.uniform("t.feat", (1024,), 0.0, 2.0))
    wout = T(synth.uniform(f"t.grouped.wout{B}", (B, C_, F_), -1.0, 1.0))
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    feat_o = feat.clone().requires_grad_(True)
    bt = {k: T(v) for k, v in b.items()}
    yo = O.audio_get_outputs(bt, feat_o, sdo, aabb, T_)
    (yo * wout).sum().backward()
    feat_d = feat.to(dev).requires_grad_(True)
    y = f.forward_queries(feat_d, bt["time_query"].to(dev), bt["mic_pose"].to(dev), bt["source_pose"].to(dev),
                          bt["rot"].to(dev), aabb, T_)
    assert y.shape == (B, C_, F_)
    assert rel_l2(y, yo) <= OUT_REL_L2
    assert float((y.detach().cpu() - yo.detach()).abs().max()) <= OUT_MAX_ABS
    (y * wout.to(dev)).sum().backward()
    assert rel_l2(feat_d.grad, feat_o.grad) <= GRAD_REL_L2
    names = list(f.state_dict())
    assert len(names) == 2 * (5 + C_)
    for name, p in f.state_dict(keep_vars=True).items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        assert rel_l2(p.grad, sdo[name].grad) <= GRAD_REL_L2, name


# ------------------------------------------------------------------------------------------------
def _parent_workspace_bytes(B, C_, F_, W=512, n_feat=1024, deterministic=False):
    """The training workspace of the layout BEFORE the per-layer dz^T slots (two ping-pong slots of 5120 + 128 rows), split layer 0."""
    M = _up(B, 128)
    np_ = [_up(n, 128) for n in (5096, 2048, 1024, 1024, W, C_ * F_)]
    take = lambda nbytes: _up(nbytes, 256)
    tot = take(M * 192 * 2) + take(256 * M * 2)
    for l in range(5):
        tot += 2 * take(M * np_[l] * 2)
    tot += take(np_[0] * 4)
    maxw = max(np_)
    tot += 2 * (take(M * maxw * 2) + take((maxw + 128) * M * 2))
    slots = M // 32 if deterministic else 1
    tot += sum(take(slots * n * 4) for n in np_) + take(256)
    if deterministic:
        tot += take(64 * n_feat * 4)
    return tot


TAIL = 1 << 20


def _field_with_guarded_workspace(C_, F_, dev):
    """A field whose workspace is the head of a larger allocation; returns (field, list of (size asked, whole buffer))."""
    f, _ = _make_field(C_, F_, dev)
    made = []

    def workspace(B, training, device, dense=False):
        from neraf_amd import _lib
        desc = f._desc_dense if dense else f._desc
        n = _lib.load().neraf_nacf_workspace_bytes(C.byref(desc), B, int(training))
        buf = torch.empty(n + TAIL, dtype=torch.uint8, device=device)
        buf[n:] = torch.arange(TAIL, device=device, dtype=torch.int32).mul_(37).add_(11).to(torch.uint8)
        made.append((n, buf))
        return buf[:n]
    f._workspace = workspace
    return f, made


def _queries(B, C_, F_, T_, dev, tag):
    b = {k: T(v).to(dev) for k, v in synth.audio_batch(B, C_, F_, T_, tag=tag).items()}
    return b, T(synth.audio_aabb()), T(synth.uniform("t.feat", (1024,), 0.0, 2.0)).to(dev)


@pytest.mark.parametrize("C_,F_,T_", [(1, 513, 60), (2, 257, 101)])
def test_workspace_covers_the_backward(dev, C_, F_, T_):
    """Forward + backward inside an allocation with a patterned tail right behind the bytes neraf_nacf_workspace_bytes asks for: the
    tail stays intact; and the size is at least what the layout with two ping-pong dz^T slots took for the same batch (every layer's
    dz^T now lives to the end of the backward; at these widths the six slots add up to exactly the two they replace)."""
    B = 200
    f, made = _field_with_guarded_workspace(C_, F_, dev)
    b, aabb, feat = _queries(B, C_, F_, T_, dev, "t.grouped.ws")
    feat.requires_grad_(True)
    y = f.forward_queries(feat, b["time_query"], b["mic_pose"], b["source_pose"], b["rot"], aabb, T_)
    y.backward(T(synth.uniform("t.grouped.ws.dout", (B, C_, F_), -1.0, 1.0)).to(dev))
    torch.cuda.synchronize()
    assert len(made) == 1
    n, buf = made[0]
    expect = torch.arange(TAIL, dtype=torch.int32).mul_(37).add_(11).to(torch.uint8)
    assert torch.equal(buf[n:].cpu(), expect), "the backward wrote behind its workspace"
    det = os.environ.get("NERAF_DETERMINISTIC", "0") not in ("", "0")
    assert n >= _parent_workspace_bytes(B, C_, F_, deterministic=det)
    for p in f.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())


def _repeat_mismatches(C_, F_, T_):
    """Three backwards on ONE workspace: dout_a, another dout in between, dout_a again.  Returns the names of the gradients (d feat and
    every parameter; "soundfield.0.weight[query]" = the query columns of dW0) whose first and third results differ in any bit."""
    dev = torch.device("cuda:0")
    B = 200
    f, _ = _make_field(C_, F_, dev)
    b, aabb, feat = _queries(B, C_, F_, T_, dev, "t.grouped.rep")
    feat.requires_grad_(True)
    y = f.forward_queries(feat, b["time_query"], b["mic_pose"], b["source_pose"], b["rot"], aabb, T_)
    da = T(synth.uniform("t.grouped.rep.a", (B, C_, F_), -1.0, 1.0)).to(dev)
    db = T(synth.uniform("t.grouped.rep.b", (B, C_, F_), -3.0, 3.0)).to(dev)
    names = [n for n, _ in f.named_parameters()]
    ps = [p for _, p in f.named_parameters()]
    runs = [[g.clone() for g in torch.autograd.grad(y, [feat] + ps, d, retain_graph=True)] for d in (da, db, da)]
    torch.cuda.synchronize()
    assert not torch.equal(runs[0][1], runs[1][1])          # the run in between really was another gradient
    n_feat = f._desc.n_feat
    bad = [name for name, g0, g2 in zip(["feat"] + names, runs[0], runs[2]) if not torch.equal(g0, g2)]
    i0 = 1 + names.index("soundfield.0.weight")
    if not torch.equal(runs[0][i0][:, n_feat:], runs[2][i0][:, n_feat:]):
        bad.append("soundfield.0.weight[query]")
    return bad


@pytest.mark.parametrize("C_,F_,T_", [(1, 513, 60), (2, 257, 101)])
def test_backward_repeats_bit_for_bit(dev, C_, F_, T_):
    """The padded tiles of the workspace are never cleared, so anything stale that reached a result would show.  In this process
    (default mode unless the suite runs under NERAF_DETERMINISTIC=1) everything the GEMMs alone produce -- every weight gradient, of
    layer 0 its query columns -- must repeat bit for bit; bias gradients, d feat and the feature columns of dW0 (the outer product of
    the layer-0 bias gradient) are fp32 atomic sums here and are checked by the deterministic-mode test below."""
    bad = _repeat_mismatches(C_, F_, T_)
    gemm_only = [n for n in bad if (n.endswith(".weight") and n != "soundfield.0.weight") or n.endswith("[query]")]
    assert not gemm_only, gemm_only
    if os.environ.get("NERAF_DETERMINISTIC", "0") not in ("", "0"):
        assert not bad, bad


def test_backward_repeats_bit_for_bit_deterministic_mode():
    """The same three backwards in a fresh process under NERAF_DETERMINISTIC=1 (the library reads the mode once per process), both head
    forms: EVERY gradient -- weights, biases, d feat -- repeats bit for bit."""
    import json
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import json, sys; sys.path[:0] = [%r, %r]; import test_gpu_nacf_grouped as t; "
            "print('BAD ' + json.dumps(t._repeat_mismatches(1, 513, 60) + t._repeat_mismatches(2, 257, 101)))" % (os.path.dirname(here), here))
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NERAF_DETERMINISTIC="1"), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-4000:]
    bad = json.loads(next(ln for ln in out.splitlines() if ln.startswith("BAD "))[len("BAD "):])
    assert bad == [], bad
