"""Continuous batching against padded batches: the bench model (bf16, D = 1024, frame sizes
16 / 4), 128 slots, 512 requests whose lengths are drawn once, uniform in [64, 256] frames.

  python tools/serve_bench.py [rounds] [n_requests] [lo] [hi]  > bench_out/serve_bench.txt

Modes, alternated in one process after a warm-up of each:
  padded    the `generate.py --batch_files` form: calls of 128 rows in request order, each padded
            to its own longest request (one-shot Generator.__call__, row_offset = first request)
  serve 32  Generator.serve(requests, 128, chunk_frames=32), stream ids = request positions
  serve 8   the same at chunk_frames=8
  session 32 / session 8   Generator.serve(..., session=True): the same plans as the chunks of
            one generation session (weights, workspace, records and graph kept between them)
All forms run 128 rows per call, so request u is the same stream in every mode: the outputs are
compared sample for sample.  Prints every round's wall time (a host clock around work that ends
on the host), then per mode the median, useful samples per second (the requests' own frames x
lookback / median) and the row-frames it ran; for serve also the plan's row-frames and calls.
Every per-call chunk re-folds the weights, carves a workspace and captures a graph,
which is what a short chunk pays for its tighter packing; a session's chunk does not.
A fifth argument `per-call` leaves the session modes out (a tree without sessions).
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

SLOTS = 128
CHUNKS = (32, 8)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    n_req = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    lo = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    hi = int(sys.argv[4]) if len(sys.argv) > 4 else 256
    import model as M
    dev = torch.device('cuda', 0)
    m, _ = bench.make_model(torch.bfloat16, seed=4242)
    m = m.to(dev)
    L = m.lookback
    rng = np.random.Generator(np.random.PCG64(2024))
    lengths = [int(v) for v in rng.integers(lo, hi + 1, n_req)]
    g = torch.Generator().manual_seed(1)
    reqs = [dict(cond=torch.rand(n, 43, generator=g), spk=u % 6) for u, n in enumerate(lengths)]
    gen = M.Generator(m, True)
    useful = sum(lengths)

    def padded(rq):
        out = {}
        for r0 in range(0, len(rq), SLOTS):
            part = rq[r0:r0 + SLOTS]
            n = max(r['cond'].shape[0] for r in part)
            cond = torch.zeros(SLOTS, n, 43)
            spk = np.zeros(SLOTS, dtype=np.int64)
            for b, r in enumerate(part):
                cond[b, :r['cond'].shape[0]] = r['cond']
                spk[b] = r['spk']
            y = gen(SLOTS, 0, cond, spk, sampler='philox', seed=5, row_offset=r0)
            for b, r in enumerate(part):
                out[r0 + b] = y[b, :r['cond'].shape[0] * L]
        return out

    def served(rq, chunk, **how):
        return dict(gen.serve(rq, SLOTS, chunk, seed=5, **how))

    modes = [('padded', padded)] + [('serve %d' % c, lambda rq, c=c: served(rq, c))
                                    for c in CHUNKS]
    if not (len(sys.argv) > 5 and sys.argv[5] == 'per-call'):
        modes += [('session %d' % c, lambda rq, c=c: served(rq, c, session=True))
                  for c in CHUNKS]
    # warm-up on a short prefix of every request (graph capture, kernel attributes); the three
    # modes give the same streams
    short = [dict(r, cond=r['cond'][:4 + u % 5]) for u, r in enumerate(reqs[:2 * SLOTS])]
    ref = None
    for name, fn in modes:
        out = fn(short)
        ref = out if ref is None else ref
        assert all(torch.equal(out[u], ref[u]) for u in ref), name
    pad_rf = sum(SLOTS * max(lengths[r0:r0 + SLOTS]) for r0 in range(0, n_req, SLOTS))
    secs = {name: [] for name, _ in modes}
    info = {}
    full = None
    for r in range(rounds):
        for name, fn in modes:
            t0 = time.perf_counter()
            out = fn(reqs)
            torch.cuda.synchronize()
            secs[name].append(time.perf_counter() - t0)
            if name != 'padded':
                info[name] = dict(gen.last_serve)
            if r == 0:
                full = out if full is None else full
                assert all(torch.equal(out[u], full[u]) for u in range(n_req)), name
            print('round %d %-10s %.4f s' % (r, name, secs[name][-1]), flush=True)
    print('%d requests, %d..%d frames (%d useful frames), %d slots, bf16 D=1024, lookback %d; '
          'outputs of all modes equal' % (n_req, min(lengths), max(lengths), useful, SLOTS, L))
    for name, _ in modes:
        v = np.array(secs[name])
        line = '%-10s median %.4f s (min %.4f max %.4f), %.0f useful samples/s' % (
            name, np.median(v), v.min(), v.max(), useful * L / np.median(v))
        if name == 'padded':
            line += ', %d row-frames in %d calls' % (pad_rf, -(-n_req // SLOTS))
        else:
            plan = M.serve_plan(lengths, SLOTS, int(name.split()[1]))
            line += ', %d row-frames in %d calls (plan: %d in %d)' % (
                info[name]['row_frames'], info[name]['calls'], sum(SLOTS * n for n, _ in plan),
                len(plan))
        print(line)


if __name__ == '__main__':
    main()
