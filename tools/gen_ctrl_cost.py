"""Cost of the sampling controls in the persistent generation loop: 128 utterances, bf16,
D = 1024 (bench.py's `gen` line), the same process and model, alternating

    off      temperature 1, top-k off      (srnn::generate, the plain kernels)
    tau      temperature 0.7 on every row  (srnn::generate_ctrl, the controlled builds)
    tau+k    temperature 0.7, top_k 16
    tau+p    temperature 0.7, top_p 0.9    (srnn::generate_ctrl_p, the level-2 builds)
    tau+k+p  temperature 0.7, top_k 16, top_p 0.9

  python tools/gen_ctrl_cost.py [n_cond] [rounds] [dtype]  > bench_out/gen_ctrl_cost.txt

Prints each call's time per generated sample (one sample = one step of all 128 rows) and, per
mode, the median and the difference to `off`.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

MODES = (('off', {}), ('tau', dict(temperature=0.7)), ('tau+k', dict(temperature=0.7, top_k=16)),
         ('tau+p', dict(temperature=0.7, top_p=0.9)),
         ('tau+k+p', dict(temperature=0.7, top_k=16, top_p=0.9)))


def main():
    n_cond = int(sys.argv[1]) if len(sys.argv) > 1 else 750
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dtype = torch.float32 if len(sys.argv) > 3 and sys.argv[3] == 'fp32' else torch.bfloat16
    import model as M
    dev = torch.device('cuda', 0)
    B = 128
    m, _ = bench.make_model(dtype, seed=4242)
    m = m.to(dev)
    cond = torch.rand(B, n_cond, 43, generator=torch.Generator().manual_seed(1))
    spk = np.arange(B) % 6
    gen = M.Generator(m, True)
    steps = n_cond * m.lookback
    for _, kw in MODES:                      # warm-up: graph capture, kernel attributes
        gen(B, 0, cond[:, :4], spk, sampler='philox', seed=5, **kw)
    torch.cuda.synchronize()
    us = {name: [] for name, _ in MODES}
    for r in range(rounds):
        for name, kw in MODES:
            t0 = time.perf_counter()
            gen(B, 0, cond, spk, sampler='philox', seed=5, **kw)
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) / steps * 1e6)
            print('round %d %-7s %.4f us/sample' % (r, name, us[name][-1]), flush=True)
    base = float(np.median(us['off']))
    for name, _ in MODES:
        v = np.array(us[name])
        print('%-7s median %.4f us/sample (min %.4f max %.4f), %+.4f vs off; %d samples x %d rows,'
              ' %s' % (name, np.median(v), v.min(), v.max(), np.median(v) - base, steps, B,
                       str(dtype).replace('torch.', '')))


if __name__ == '__main__':
    main()
