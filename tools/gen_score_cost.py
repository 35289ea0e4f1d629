"""Cost of a scored generation call in the persistent loop: 128 utterances, D = 1024 (bench.py's
`gen` model), the same process and model, alternating

    off      no scores, no log-probs            (srnn::generate, the plain kernels)
    tau      temperature 0.7 on every row       (the level-1 builds, for comparison)
    scored   return_scores=True                 (srnn::generate_scored, the level-3 builds:
                                                 8 bytes per row-step)
    logp     return_logp=True                   (the plain kernels with the dense (T, B, 256)
                                                 buffer: 1 KiB per row-step)

  python tools/gen_score_cost.py [n_cond] [rounds] [dtype]  > bench_out/gen_score_cost.txt

Prints each call's time per generated sample (one sample = one step of all 128 rows) and, per
mode, the median and the difference to `off` (DESIGN §6 "Scores").  The dense buffer of the
`logp` mode takes n_cond * lookback * 128 KiB on the device, twice while it is re-laid: keep
n_cond moderate.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

MODES = (('off', {}), ('tau', dict(temperature=0.7)), ('scored', dict(return_scores=True)),
         ('logp', dict(return_logp=True)))


def main():
    n_cond = int(sys.argv[1]) if len(sys.argv) > 1 else 120
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
            res = gen(B, 0, cond, spk, sampler='philox', seed=5, **kw)
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) / steps * 1e6)
            del res
            print('round %d %-7s %.4f us/sample' % (r, name, us[name][-1]), flush=True)
    base = float(np.median(us['off']))
    for name, _ in MODES:
        v = np.array(us[name])
        print('%-7s median %.4f us/sample (min %.4f max %.4f), %+.4f vs off; %d samples x %d rows,'
              ' %s' % (name, np.median(v), v.min(), v.max(), np.median(v) - base, steps, B,
                       str(dtype).replace('torch.', '')))


if __name__ == '__main__':
    main()
