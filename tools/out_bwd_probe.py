"""Per-call GPU time of the fused output-layer backward (srnn_mlp_out_bwd, with db_out) against
the separate calls it replaces (masked da2 GEMM with the column-sum epilogue, dz^T . a2 GEMM,
column sum of dz), bf16, Q = 256 (run from the repo root; profiles/r08_out_bwd_ab.txt):

  python3 tools/out_bwd_probe.py            # M = 65536, 131072, 524288 at D = 1024: HIP events
                                            # around each call, median of 10
  python3 tools/out_bwd_probe.py --graph    # small shapes: 20 calls per captured graph (launch
                                            # overhead off the clock), median of 7 replays
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'jalil-saboorizadeh-multi-speaker-neural-vocoder_amd'))
import torch  # noqa: E402
import samplernn_hip as H  # noqa: E402

Q = 256


def operands(M, D):
    dz = (torch.randn((M, Q), device='cuda') * 0.05).bfloat16()
    a2 = (torch.randn((M, D), device='cuda') * 0.5).clamp_(min=0).bfloat16()
    wt = (torch.randn((D, Q), device='cuda') * 0.03).bfloat16()
    return dz, a2, wt, torch.empty((M // 128, D), device='cuda')


def da2_call(dz, a2, wt, csp):
    return H.gemm(dz, wt, transB=True, mask=a2, out_dtype=torch.bfloat16,
                  epilogue=H.GemmEpilogue(csum=csp))


def timed(fn, reps=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def graph_time(fn, n=20):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / n * 1e3)
    ts.sort()
    return ts[3]


def main():
    if '--graph' in sys.argv[1:]:
        for M, D in ((4096, 256), (4096, 1024), (8192, 1024), (16384, 256), (16384, 1024),
                     (32768, 1024), (65536, 1024)):
            dz, a2, wt, csp = operands(M, D)

            def sep():
                da2_call(dz, a2, wt, csp)
                H.gemm(dz, a2, transA=True)
                H.colsum(dz, M, Q)
            f = graph_time(lambda: H.mlp_out_bwd(dz, a2, wt))
            u = graph_time(sep)
            print('M %6d D %4d: fused %7.1f us, separate %7.1f us' % (M, D, f, u), flush=True)
        return
    D = 1024
    for M in (65536, 131072, 524288):
        dz, a2, wt, csp = operands(M, D)
        f = timed(lambda: H.mlp_out_bwd(dz, a2, wt))
        u1 = timed(lambda: da2_call(dz, a2, wt, csp))
        u2 = timed(lambda: H.gemm(dz, a2, transA=True))
        u3 = timed(lambda: H.colsum(dz, M, Q))
        gb = (M * Q * 2 + 2 * M * D * 2) / 1e9
        print('M %7d: fused %.3f ms (min %.3f max %.3f; %.2f TB/s of %.2f GB) | separate da2 %.3f '
              '+ dW %.3f + colsum %.3f = %.3f ms'
              % (M, f[0], f[1], f[2], gb / f[0], gb, u1[0], u2[0], u3[0], u1[0] + u2[0] + u3[0]),
              flush=True)
        del dz, a2, wt, csp


if __name__ == '__main__':
    main()
