#!/usr/bin/env python3
"""A/B of the streaming GEMM body (gemm_f16_nt_stream_kernel, body = 1) against the tile bodies of the same build (body = 2) on the
plain-GEMM shapes of ResNet3D layer 1, with the method of tools/small_gemm_bench.py: a dependent chain of NL launches inside a
replayed graph, the A operand, the weights and the results rotating over NB buffers each (NB x (A + C) is far beyond the L2 and the
MALL, so every launch streams from HBM as it does in the training step), statistics accumulated as the encoder asks for them
(atomics into 16 replicas 1024 floats apart).

    python3 tools/stream_gemm_bench.py [M ...]        (default M = 32768; further M sweep the dispatch threshold)
"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from neraf_amd import _lib
lib = _lib.load(); h = _lib.ctx(0)
dev = torch.device("cuda:0")
# (N, K, add16, statistics): the rows of the layer-1 table -- forward 64 -> 256, its dgrad with the residual gradient added,
# forward 256 -> 64 and its dgrads, the 64 -> 64 pair; then the three (N, K) the body serves that layer 1 does not use
SHAPES = [(256, 64, 0, 1), (256, 64, 1, 0), (64, 256, 0, 1), (64, 256, 1, 0), (64, 64, 0, 1), (64, 64, 0, 0), (128, 128, 0, 1), (128, 64, 0, 1),
          (64, 128, 0, 1),
          # the two shapes that run as two column slices of 32 KiB of B each: layer 2's first 1x1x1 convolution (256 -> 128 on the
          # 32768 voxels of layer 1's output) and its dgrad
          (128, 256, 0, 1), (256, 128, 0, 0)]
NB = int(os.environ.get("NB_BUFFERS", "8"))
NL, R = 24, 20
Ms = [int(a) for a in sys.argv[1:]] or [32768]
side = torch.cuda.Stream()
for M in Ms:
    for N, K, add, st in SHAPES:
        As = [(torch.rand(M, K, device=dev) - 0.5).half() for _ in range(NB)]
        Bs = [(torch.rand(N, K, device=dev) - 0.5).half() for _ in range(NB)]
        Ds = [(torch.rand(M, N, device=dev) - 0.5).half() for _ in range(NB)] if add else None
        Cs = [torch.empty(M, N, dtype=torch.float16, device=dev) for _ in range(NB)]
        stats = torch.zeros(2, 16 * 1024, device=dev)
        us = {}
        for body in (2, 1):
            def chain(s):
                for i in range(NL):
                    j = i % NB
                    _lib.check(lib.neraf_gemm_f16_stream(h, As[j].data_ptr(), K, Bs[j].data_ptr(), K, M, N, K, M, N, 1.0, None,
                                                         Ds[j].data_ptr() if add else None, N, Cs[j].data_ptr(), N, None, 0, None, 0,
                                                         stats[0].data_ptr() if st else None, stats[1].data_ptr() if st else None, 16, 1024, 0,
                                                         body, 0, C.c_void_p(s)))
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
            us[body] = e0.elapsed_time(e1) * 1e3 / (R * NL)
        mb = (M * K + N * K + M * N * (2 if add else 1)) * 2 / 1e6
        print(f"M{M:6d} N{N:4d} K{K:4d} add16={add} stats={st}: tile {us[2]:6.2f} us   stream {us[1]:6.2f} us   x{us[2] / us[1]:.2f}   "
              f"{mb:5.1f} MB -> {mb / us[1]:.2f} TB/s", flush=True)
