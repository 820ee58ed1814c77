"""Interleaved A/B of libdgx.so builds on the split-K weight-gradient (TN) GEMMs,
through the C ABI: dgx_gemm_lds_bf16(tn = 1, SLAB) at the shapes the DGCNN step
launches (conv5 dW and the dW of EdgeConv blocks 2-4), hipEvent time per launch,
median over the rounds, once with the operands just written ("hot": in the step
dZ is freshly written) and once after a 1 GiB fill pushed them out of the caches
("cold"). Every build's slabs are compared bit for bit with the first build's.

  python tools/tn_ab.py [--rounds 15] [--configs cfg2,cfg3,cfg5] [--once] LIB [LIB ...]

--once: one hot launch per shape and library plus one slab reduce (the run a
counter pass profiles). Diagnostic (tools/), not part of the product."""
import argparse
import ctypes
import os
import statistics

import torch

ROWS = {"cfg2": 32 * 1024, "cfg3": 32 * 2048, "cfg5": 24 * 4096}
# (name, M, N, ld of B): A = dZ / dPQ (R x M, dense), B = a column slice of the bf16 concat (R x 512)
SHAPES = (("conv5 1024x512", 1024, 512, 512), ("block4 512x128", 512, 128, 512),
          ("block3 256x64", 256, 64, 512), ("block2 128x64", 128, 64, 512))
SLAB_CAP = 8 << 20


def vp(x):
    return ctypes.c_void_p(x)


def load(path):
    L = ctypes.CDLL(os.path.realpath(path))
    L.dgx_gemm_lds_bf16.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64] + \
        [ctypes.c_int] * 7 + [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                              ctypes.c_void_p]
    L.dgx_slab_reduce_f32.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_int64,
                                                                               ctypes.c_void_p]
    return L


def splits_of(L, M, N, R):
    s = L.dgx_gemm_splits(M, N, R)
    if M * N * 4 < (1 << 20):
        s = max(1, min(s, SLAB_CAP // (M * N * 4)))
    return s, L.dgx_gemm_lds_slabs(R, s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--configs", default="cfg2")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("libs", nargs="+")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    names = [os.path.basename(p) for p in a.libs]
    libs = [load(p) for p in a.libs]
    st = vp(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.Generator(device=dev).manual_seed(1)
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    for cfg in a.configs.split(","):
        R = ROWS[cfg]
        for what, M, N, ldb in SHAPES:
            src_a = torch.randn(R, M, generator=g, device=dev).to(torch.bfloat16)
            src_b = torch.randn(R, ldb, generator=g, device=dev).to(torch.bfloat16)
            A, B = torch.empty_like(src_a), torch.empty_like(src_b)
            S, used = splits_of(libs[0], M, N, R)
            slabs = [torch.empty(used, M, N, device=dev) for _ in libs]
            out = torch.empty(M, N, device=dev)

            def launch(i):
                rc = libs[i].dgx_gemm_lds_bf16(vp(A.data_ptr()), M, vp(B.data_ptr()), ldb, 1, M, N, R, R, 3, S,
                                               vp(slabs[i].data_ptr()), N, None, None, 0, st)
                assert rc == 0, (names[i], what, rc)

            if a.once:
                A.copy_(src_a), B.copy_(src_b)
                for i in range(len(libs)):
                    launch(i)
                    libs[i].dgx_slab_reduce_f32(vp(slabs[i].data_ptr()), used, M, N, M, vp(out.data_ptr()), N, st)
                torch.cuda.synchronize()
                continue
            times = {(i, m): [] for i in range(len(libs)) for m in ("hot", "cold")}
            for r in range(a.rounds + 1):          # round 0 warms up
                for mode in ("hot", "cold"):
                    for i in range(len(libs)):
                        A.copy_(src_a), B.copy_(src_b)
                        if mode == "cold":
                            flush.fill_(1.0)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        launch(i)
                        e1.record()
                        torch.cuda.synchronize()
                        if r:
                            times[(i, mode)].append(e0.elapsed_time(e1) * 1e3)
            same = [bool(torch.equal(slabs[0], s)) for s in slabs]
            print(f"{cfg} {what} R={R} splits={S} slabs={used}")
            for i, n in enumerate(names):
                h, c = times[(i, "hot")], times[(i, "cold")]
                print(f"  {n:28s} hot {statistics.median(h):7.1f} us (min {min(h):6.1f})  cold "
                      f"{statistics.median(c):7.1f} us (min {min(c):6.1f})  slabs "
                      f"{'bit-equal' if same[i] else 'DIFFER'} to {names[0]}")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
