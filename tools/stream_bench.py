"""Cost of streaming generation in chunks: 128 utterances, bf16, D = 1024 (bench.py's `gen`
line), the same process and model, alternating the one-shot Generator.__call__ with
Generator.stream at chunk_frames 2, 8 and 32 over the same utterance, per call (`chunk N`) and
through one generation session (`session N`: Generator.stream(session=True)).

  python tools/stream_bench.py [n_cond] [rounds] [dtype] [one-shot]  > bench_out/stream_bench.txt

Every call re-folds the weights, carves a workspace and (from its second two-period block on)
captures a graph, so a chunk pays a set-up cost the one-shot call pays once; a session keeps
all of that between its chunks (and is opened and closed inside the timed region).  Prints each
call's time per generation step (one step = one sample of all 128 rows; a host clock around
work that ends in a device synchronise, after a warm-up of every mode) and, per mode, the
median, the spread and the overhead per chunk = (t_stream - t_one_shot) / chunks, from the
medians and per round against the same round's one-shot call.
A fourth argument `one-shot` times the one-shot call alone (any commit: it needs no stream),
`per-call` leaves the session modes out (a tree without sessions).
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

CHUNKS = (2, 8, 32)


def main():
    n_cond = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dtype = torch.float32 if len(sys.argv) > 3 and sys.argv[3] == 'fp32' else torch.bfloat16
    only = len(sys.argv) > 4 and sys.argv[4] == 'one-shot'
    per_call = len(sys.argv) > 4 and sys.argv[4] == 'per-call'
    import model as M
    dev = torch.device('cuda', 0)
    B = 128
    m, _ = bench.make_model(dtype, seed=4242)
    m = m.to(dev)
    cond = torch.rand(B, n_cond, 43, generator=torch.Generator().manual_seed(1))
    spk = np.arange(B) % 6
    gen = M.Generator(m, True)
    steps = n_cond * m.lookback
    kw = dict(sampler='philox', seed=5)

    def one_shot(c):
        return gen(B, 0, c, spk, **kw)

    def streamed(c, chunk, **how):
        return torch.cat(list(gen.stream(B, c, spk, chunk, **how, **kw)), 1)

    modes = [('one-shot', one_shot)]
    if not only:
        modes += [('chunk %d' % c, lambda x, c=c: streamed(x, c)) for c in CHUNKS]
    if not only and not per_call:
        modes += [('session %d' % c, lambda x, c=c: streamed(x, c, session=True))
                  for c in CHUNKS]
    ref = None
    for name, fn in modes:                   # warm-up (graph capture, kernel attributes), and
        out = fn(cond[:, :8])                # the streams are the one-shot stream
        ref = out if ref is None else ref
        assert torch.equal(out, ref), name
    torch.cuda.synchronize()
    us = {name: [] for name, _ in modes}
    for r in range(rounds):
        for name, fn in modes:
            t0 = time.perf_counter()
            fn(cond)
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) / steps * 1e6)
            print('round %d %-10s %.4f us/step' % (r, name, us[name][-1]), flush=True)
    base = float(np.median(us['one-shot']))
    for name, _ in modes:
        v = np.array(us[name])
        line = '%-10s median %.4f us/step (min %.4f max %.4f)' % (name, np.median(v), v.min(),
                                                                  v.max())
        if name != 'one-shot':
            n_chunks = -(-n_cond // int(name.split()[1]))
            per = (v - np.array(us['one-shot'])) * steps / n_chunks
            line += (', %+.4f vs one-shot, %.1f us per chunk over %d chunks (per round: median '
                     '%.1f, min %.1f, max %.1f)' % (
                         np.median(v) - base, (np.median(v) - base) * steps / n_chunks, n_chunks,
                         np.median(per), per.min(), per.max()))
        print(line + '; %d steps x %d rows, %s' % (steps, B, str(dtype).replace('torch.', '')))


if __name__ == '__main__':
    main()
