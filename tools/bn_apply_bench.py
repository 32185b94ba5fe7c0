#!/usr/bin/env python3
"""A/B of the two forms of the forward BatchNorm pass (neraf_debug_bn_apply: form 0 = bn_apply_kernel, 1 = bn_apply_tile_kernel) over
the shapes the encoder runs on the 7 x 128^3 grid, with the method of tools/stream_gemm_bench.py: a chain of NL launches inside a
replayed graph, operands and results rotating over NB buffers (far beyond the L2 and the MALL at the layer-1 sizes), train-mode
statistics in as many replicas as the encoder uses at that size.  Sets kBnTileMinChunks (csrc/resnet3d_common.h).

    python3 tools/bn_apply_bench.py [form ...]        (default forms 0 1)
"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from neraf_amd import _lib
lib = _lib.load(); h = _lib.ctx(0)
dev = torch.device("cuda:0")
# (M, C, second operand, replicas): layer 1 (32768 voxels), layer 2 (4096), layer 3 (512)
SHAPES = [(32768, 64, "none", 16), (32768, 128, "none", 16), (32768, 256, "residual", 16), (32768, 256, "bn", 16),
          (4096, 128, "none", 4), (4096, 256, "none", 4), (4096, 512, "residual", 4), (4096, 512, "bn", 4),
          (512, 256, "none", 1), (512, 1024, "residual", 1), (512, 1024, "bn", 1)]
NB = int(os.environ.get("NB_BUFFERS", "8"))
NL, R = 24, 20
forms = [int(a) for a in sys.argv[1:]] or [0, 1]
side = torch.cuda.Stream()
for M, Cc, second, rep in SHAPES:
    xs = [(torch.rand(M, Cc, device=dev) - 0.5).half() for _ in range(NB)]
    rs = [(torch.rand(M, Cc, device=dev) - 0.5).half() for _ in range(NB)] if second != "none" else None
    outs = [torch.empty(M, Cc, dtype=torch.float16, device=dev) for _ in range(NB)]
    stats = torch.rand(2, 16 * 1024, device=dev) * M
    par = [torch.rand(Cc, device=dev) + 0.5 for _ in range(4)]
    fin = torch.zeros(2, 2 * 1024, device=dev)
    bn5 = [(C.c_void_p * 5)(stats[k].data_ptr(), *[p.data_ptr() for p in par]) for k in (0, 1)]
    us = {}
    for form in forms:
        def chain(s):
            for i in range(NL):
                j = i % NB
                _lib.check(lib.neraf_debug_bn_apply(h, xs[j].data_ptr(), bn5[0], rep, rs[j].data_ptr() if second == "bn" else None,
                                                    bn5[1] if second == "bn" else None, rep if second == "bn" else 0,
                                                    rs[j].data_ptr() if second == "residual" else None, M, M, Cc, 1, fin[0].data_ptr(),
                                                    fin[1].data_ptr(), outs[j].data_ptr(), form, C.c_void_p(s)))
        with torch.cuda.stream(side):
            chain(side.cuda_stream)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                chain(torch.cuda.current_stream().cuda_stream)
        for _ in range(3): g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for _ in range(R): g.replay()
        e1.record(); torch.cuda.synchronize()
        us[form] = e0.elapsed_time(e1) * 1e3 / (R * NL)
    mb = M * Cc * 2 * (3 if second != "none" else 2) / 1e6
    print(f"M{M:6d} C{Cc:5d} {second:>8s} rep={rep:2d} {mb:6.2f} MB: " +
          "   ".join(f"form {f} {us[f]:6.2f} us {mb / us[f]:5.2f} TB/s" for f in forms), flush=True)
