"""Per-row nucleus (top-p) sampling (csrc/sampler.hpp, the (tau, k, p) sample_row_ctrl;
Generator.__call__(top_p=)) and the stand-alone row sampler samplernn_hip.sample_rows.

* direct: sample_rows on the fixed synthetic rows of nucleus_ref.py (chosen logits, replayed and
  adversarial noise) returns exactly the reference's indices, none left out; log-probs; p = 1
  rows; the plain level against a plain generation run; the Philox distribution;
* loop: every index the persistent loop and the per-sample kernels draw with (tau, k, p) mixed
  per row is the definition's, up to the device's mass error at the cut-off; both paths agree;
* bit-identity: a p = 1 row in a mixed batch, and the level-2 builds given all-default arrays
  against the plain loop at D = 1024;
* plumbing: rank-sharded generation, generate.py --top_p, the registered ops, the C symbols.
"""
import os
import sys

import numpy as np
import pytest
import torch

import nucleus_ref as N
import recipe
import sampling_ref as R
from test_gpu_generation import build, generate

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), 'jalil-saboorizadeh-multi-speaker-neural-vocoder_amd')


def _dev(S):
    return (S['logits'].to(DEV), S['noise'].to(DEV),
            torch.tensor(S['tau'], dtype=torch.float32, device=DEV),
            torch.tensor(S['k'], dtype=torch.int32, device=DEV),
            torch.tensor(S['p'], dtype=torch.float32, device=DEV))


# ------------------------------------------------------------------ direct: sample_rows
def test_sample_rows_is_the_reference_on_the_synthetic_rows(hip):
    S = N.synthetic()
    z, q, tau, k, p = _dev(S)
    idx, lp = hip.sample_rows(z, q, temperature=tau, top_k=k, top_p=p, return_logp=True)
    assert idx.dtype == torch.int64 and idx.shape == (N.ROWS,) and lp.shape == (N.ROWS, 256)
    got = idx.cpu()
    bad = (got != S['x']).nonzero().flatten().tolist()
    assert not bad, [(b, S['p'][b], S['tau'][b], S['k'][b], int(got[b]), int(S['x'][b]),
                      bool(S['inside'][b]), int(S['adv'][b])) for b in bad]
    torch.testing.assert_close(lp.cpu(), torch.log_softmax(S['logits'], -1), atol=1e-5, rtol=0)
    # a strided view (leading dimension 320) draws the same
    wide = torch.zeros(N.ROWS, 320, device=DEV)
    wide[:, :256] = z
    assert torch.equal(hip.sample_rows(wide[:, :256], q, temperature=tau, top_k=k, top_p=p), idx)
    # the controls one array at a time: a null array is that control at its default
    on = [b for b in range(N.ROWS) if S['k'][b] == 0 and S['tau'][b] == 1.0]
    sub = torch.tensor(on, device=DEV)
    assert torch.equal(hip.sample_rows(z[sub].contiguous(), q[sub].contiguous(),
                                       top_p=p[sub].contiguous()), idx[sub])


def test_sample_rows_p_one_rows_are_the_call_without_top_p(hip):
    S = N.synthetic()
    z, q, tau, k, p = _dev(S)
    with_p = hip.sample_rows(z, q, temperature=tau, top_k=k, top_p=p)
    without = hip.sample_rows(z, q, temperature=tau, top_k=k)
    off = torch.tensor([pp == 1.0 or t == 0.0 for pp, t in zip(S['p'], S['tau'])], device=DEV)
    assert int(off.sum()) >= 13
    assert torch.equal(with_p[off], without[off])
    assert not torch.equal(with_p[~off], without[~off])


def test_sample_rows_plain_level_reproduces_a_generation_run(hip):
    cfg = dict(recipe.CONFIGS['t3'], dim=64)
    m, _ = build(cfg, 7, torch.float32)
    B, n_cond = 8, 1
    cond = recipe.synth_cond((B, n_cond, cfg['cond_dim']), 4)
    spk = np.arange(B) % cfg['spk_dim']
    noise = torch.from_numpy(recipe.synth_noise((n_cond * 64, B, 256), 9))
    seq, lp = generate(m, B, cond, spk, True, noise=noise)          # lp (B, T, Q)
    T = lp.shape[1]
    rows = lp.permute(1, 0, 2).reshape(T * B, 256).contiguous()     # row t * B + b
    idx, lp2 = hip.sample_rows(rows.to(DEV), noise.reshape(T * B, 256).to(DEV), return_logp=True)
    sc = rows.double() - torch.log(noise.reshape(T * B, 256).double())
    top = torch.topk(sc, 2, dim=-1).values
    clear = (top[:, 0] - top[:, 1]) >= 1e-4
    want = seq[:, m.lookback:].t().reshape(-1)
    assert clear.float().mean() > 0.99
    assert torch.equal(idx.cpu()[clear], want[clear])
    torch.testing.assert_close(lp2.cpu(), rows, atol=1e-5, rtol=0)


def test_sample_rows_philox_distribution(hip):
    """128 identical rows x 8 seeds, tau = 0.7, p = 0.9 on the synthetic distribution: all 1024
    draws lie in N and the counts follow the renormalised tempered softmax within 5 binomial
    sigma.  Philox is counter-based: a fixed outcome.  Rows [row0, row0 + n) of a call draw what
    rows [0, n) of a call at that offset draw."""
    S = N.synthetic()
    z1 = S['logits'][1:2]
    tau, pp = 0.7, 0.9
    inN, gap, _ = N.nucleus(z1, [tau], [0], [pp])
    assert float(gap[0]) >= 1e-3
    B = 128
    z = z1.expand(B, 256).contiguous().to(DEV)
    t = torch.full((B,), tau, device=DEV)
    p = torch.full((B,), pp, device=DEV)
    draws = torch.cat([hip.sample_rows(z, None, seed=s, step=3, temperature=t, top_p=p).cpu()
                       for s in range(8)])
    assert draws.numel() == 1024
    members = inN[0].nonzero().flatten()
    assert bool(inN[0][draws].all()), 'draws outside the nucleus'
    w = torch.softmax(z1[0, members].double() / tau, 0)
    counts = torch.stack([(draws == j).sum() for j in members]).double()
    n = draws.numel()
    sigma = torch.sqrt(n * w * (1 - w))
    print('nucleus of %d, p' % members.numel(), w.tolist(), 'counts', counts.tolist())
    assert ((counts - n * w).abs() <= 5 * sigma).all(), (counts.tolist(), (n * w).tolist())
    part = hip.sample_rows(z[:40], None, seed=2, row0=50, step=3, temperature=t[:40], top_p=p[:40])
    assert torch.equal(part.cpu(), draws[2 * B + 50: 2 * B + 90])


def test_sample_rows_rejects_bad_arguments(hip):
    z = torch.zeros(4, 256, device=DEV)
    with pytest.raises(ValueError):
        hip.sample_rows(torch.zeros(4, 255, device=DEV))
    with pytest.raises(ValueError):
        hip.sample_rows(z, torch.ones(3, 256, device=DEV))
    with pytest.raises(ValueError):
        hip.sample_rows(z, top_p=torch.ones(4, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        hip.sample_rows(z, top_k=torch.ones(4, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        hip.sample_rows(z.double())


# ------------------------------------------------------------------ the loop, fp32
@pytest.fixture(scope='module')
def fixed(hip):
    """The definition test's fixed inputs, run once per path: (tau, k, p) mixed per row, and
    the uncontrolled run."""
    cfg = dict(recipe.CONFIGS['t3'], dim=64)
    m, _ = build(cfg, 7, torch.float32)
    B, n_cond = 8, 3
    assert hip.gen_persistent_rows(torch.float32, B, 64, 16, ctrl=2) > 0     # the level-2 plan
    cond = recipe.synth_cond((B, n_cond, cfg['cond_dim']), 4)
    spk = np.arange(B) % cfg['spk_dim']
    noise = torch.from_numpy(recipe.synth_noise((192, B, 256), 9))
    tau, k, p = N.controls(B)
    out = {'noise': noise, 'tau': tau, 'k': k, 'p': p, 'L': m.lookback}
    for name, persistent in (('persistent', True), ('per_sample', False)):
        out[name] = generate(m, B, cond, spk, persistent, noise=noise, temperature=tau, top_k=k,
                             top_p=p)
        out[name + '_plain'] = generate(m, B, cond, spk, persistent, noise=noise)
    return out


@pytest.mark.parametrize('path', ['persistent', 'per_sample'])
def test_loop_draws_are_the_definition_fp32(fixed, path):
    seq, lp = fixed[path]
    N.check_self_consistent(lp, fixed['noise'], seq, fixed['L'], fixed['tau'], fixed['k'],
                            fixed['p'])


def test_loop_paths_agree(fixed):
    s1, l1 = fixed['persistent']
    s0, l0 = fixed['per_sample']
    assert torch.equal(s1, s0)
    torch.testing.assert_close(l1, l0, atol=1e-4, rtol=0)


@pytest.mark.parametrize('path', ['persistent', 'per_sample'])
def test_p_one_row_is_its_uncontrolled_self(fixed, path):
    seq, lp = fixed[path]
    seq0, lp0 = fixed[path + '_plain']
    assert fixed['p'][0] == 1.0 and fixed['tau'][0] == 1.0 and fixed['k'][0] == 0
    assert torch.equal(seq[0], seq0[0])
    assert torch.equal(lp[0], lp0[0])
    assert not torch.equal(seq, seq0)          # (the controls did change the other rows)


def test_top_p_of_ones_takes_todays_path(hip):
    """top_p = 1 on every row is no nucleus array: the call is the (tau, k) one, bit for bit."""
    cfg = dict(recipe.CONFIGS['t3'], dim=64)
    m, _ = build(cfg, 7, torch.float32)
    B = 8
    cond = recipe.synth_cond((B, 2, cfg['cond_dim']), 4)
    spk = np.arange(B) % cfg['spk_dim']
    tau, k = R.controls(B)
    a = generate(m, B, cond, spk, True, sampler='philox', seed=3, temperature=tau, top_k=k)
    b = generate(m, B, cond, spk, True, sampler='philox', seed=3, temperature=tau, top_k=k,
                 top_p=np.ones(B))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # p alone (tau and k materialised at their defaults) draws inside the nucleus
    seq, lp = generate(m, B, cond, spk, True, sampler='philox', seed=3, top_p=0.5)
    inN, _, _ = N.nucleus(lp.permute(1, 0, 2), [1.0] * B, [0] * B, [0.5 + 2e-4] * B)
    x = seq[:, m.lookback:].t().unsqueeze(-1)
    assert bool(torch.gather(inN, -1, x).all())
    assert not torch.equal(seq, generate(m, B, cond, spk, True, sampler='philox', seed=3)[0])


# ------------------------------------------------------------------ bf16 / fp32, D = 1024
@pytest.mark.parametrize('B,tg', [(128, '1'), (128, '0'), (9, '1'), (9, '0')])
def test_loop_draws_are_the_definition_bf16_d1024(hip, monkeypatch, B, tg):
    monkeypatch.setenv('SRNN_GEN_TICK_GEMM', tg)
    cfg = recipe.CONFIGS['big']
    m, _ = build(cfg, 11, torch.bfloat16)
    assert hip.gen_persistent_rows(torch.bfloat16, B, 1024, 16, ctrl=2) > 0
    n_cond = 2
    cond = recipe.synth_cond((B, n_cond, cfg['cond_dim']), 5)
    spk = np.arange(B) % cfg['spk_dim']
    noise = torch.from_numpy(recipe.synth_noise((n_cond * 64, B, 256), 3))
    tau, k, p = N.controls(B)
    seq, lp = generate(m, B, cond, spk, True, noise=noise, temperature=tau, top_k=k, top_p=p)
    N.check_self_consistent(lp, noise, seq, m.lookback, tau, k, p)


@pytest.mark.parametrize('dtype,B,tg', [
    (torch.bfloat16, 128, '1'), (torch.bfloat16, 128, '0'), (torch.bfloat16, 9, '1'),
    (torch.bfloat16, 9, '0'), (torch.float32, 9, '1')])
def test_level2_builds_at_defaults_are_the_plain_loop_d1024(hip, monkeypatch, dtype, B, tg):
    """Like the level-1 builds, the level-2 builds load the next tick's gate operands after the
    sample loop: given all-default arrays they must reproduce the plain loop bit for bit, index
    stream and log-probs, over 8 bottom ticks."""
    import model as M
    monkeypatch.setenv('SRNN_GEN_TICK_GEMM', tg)
    cfg = recipe.CONFIGS['big']
    m, _ = build(cfg, 11, dtype)
    assert hip.gen_persistent_rows(dtype, B, 1024, 16) > 0
    assert hip.gen_persistent_rows(dtype, B, 1024, 16, ctrl=2) > 0
    n_cond = 2
    cond = torch.from_numpy(recipe.synth_cond((B, n_cond, cfg['cond_dim']), 5)).to(
        DEV, torch.float32).contiguous()
    spk = torch.from_numpy(np.arange(B) % cfg['spk_dim']).to(DEV)
    noise = torch.from_numpy(recipe.synth_noise((n_cond * 64, B, 256), 3)).to(DEV)
    weights, meta = M.generation_weights(m)
    rb = M.top_row_bias(m, spk)
    args = (weights, meta, cond, rb, noise, 0, 0, 1, True)
    s0, l0 = torch.ops.srnn.generate(*args)
    s1, l1 = torch.ops.srnn.generate_ctrl_p(
        *args, torch.ones(B, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV),
        torch.ones(B, device=DEV))
    assert torch.equal(s1, s0)
    assert torch.equal(l1, l0)
    assert torch.isfinite(l0).all()


# ------------------------------------------------------------------ plumbing
def _shard_worker(rank, world, port, q):
    try:
        sys.path[:0] = [HERE, os.path.join(HERE, 'golden'), PKG]
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                          WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
        import distributed as D
        import model as M
        import samplernn_hip as H
        from test_gpu_parity import build as pbuild
        D.init(backend='gloo')
        H.lib()
        cfg = recipe.CONFIGS['t3']
        m, _ = pbuild(cfg, recipe.make_weights(cfg, 51), torch.float32)
        n, n_cond = 6, 2
        cond = recipe.synth_cond((n, n_cond, cfg['cond_dim']), 6)
        spk = np.arange(n) % cfg['spk_dim']
        # rank 0's rows hold the tightest nucleus, rank 1's a p = 1 row among nucleus rows
        tau = [1.0, 0.6, 1.0, 1.0, 0.0, 1.4]
        k = [0, 0, 12, 0, 0, 3]
        p = [1.0, 0.3, 0.9, 0.5, 0.7, 1.0]
        out = M.shard_generate(M.Generator(m, True), n, cond, spk, 99, sampler='philox',
                               temperature=tau, top_k=k, top_p=p)
        full = None
        if rank == 0:
            full = M.Generator(m, True)(n, 0, cond, spk, sampler='philox', seed=99,
                                        temperature=tau, top_k=k, top_p=p).numpy()
            nop = M.Generator(m, True)(n, 0, cond, spk, sampler='philox', seed=99,
                                       temperature=tau, top_k=k).numpy()
            assert np.array_equal(full[0], nop[0]) and np.array_equal(full[5], nop[5])
            assert not np.array_equal(full[1:4], nop[1:4])
        q.put((rank, out.numpy(), full, None))
        D.barrier()
        import torch.distributed as dist
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, None, None, traceback.format_exc()))
        raise


def test_sharded_generation_with_top_p_reproduces_single_process(hip):
    from test_gpu_distributed import _spawn
    got = _spawn(_shard_worker, ())
    full = got[0][1]
    for rank in (0, 1):
        assert np.array_equal(got[rank][0], full), rank


def test_generate_cli_top_p(hip, tmp_path):
    """generate.py --top_p 1e-6 --temperature 1: the nucleus is the most probable class alone, so
    the audio is the same whatever the --seed, and not the default run's.  A tiny untrained
    model saved as a checkpoint (no training run needed)."""
    import model as M
    from scipy.io import wavfile
    from test_cpu_data import _write_corpus
    from test_gpu_sampling_controls import _run
    root = str(tmp_path) + '/'
    files = ['72e000', '75v000']
    _, cond = _write_corpus(root, files, frames=(5, 6))
    for s in ('72', '75'):
        os.symlink(tmp_path, os.path.join(cond, 'spk' + s))
    (tmp_path / 'generate_cond_gina.list').write_text('\n'.join(files) + '\n')
    (tmp_path / 'generate_spk_gina.list').write_text('72\n75\n')
    os.makedirs(tmp_path / 'npy_datasets')
    np.save(tmp_path / 'npy_datasets' / 'spk_id.npy', np.array(['72', '75']))
    np.save(tmp_path / 'npy_datasets' / 'min_max_joint.npy',
            np.stack([np.full(43, -5.0), np.full(43, 7000.0)]))
    torch.manual_seed(3)
    net = M.SampleRNN([20, 4], 1, 32, True, 256, True, False, 43, 2)
    ck = 'results/exp:C/checkpoints/ep1-it1'
    os.makedirs(tmp_path / 'results' / 'exp:C' / 'checkpoints')
    os.makedirs(tmp_path / 'results' / 'exp:C' / 'samples')
    torch.save(M.Predictor(net).state_dict(), str(tmp_path / ck))
    base = [os.path.join(PKG, 'generate.py'), '--model', ck, '--datasets_path', root,
            '--cond_set', 'cond/', '--frame_sizes', '20', '4', '--n_rnn', '1', '--dim', '32',
            '--sampler', 'philox', '--batch_files', 'true']

    def audio(extra):
        _run(base + extra, str(tmp_path))
        out = []
        for f, s in zip(files, ('72', '75')):
            name = tmp_path / 'results' / 'exp:C' / 'samples' / (
                'ep1-it1_file-' + f + '_spk-' + s + '.wav')
            sr, y = wavfile.read(str(name))
            assert sr == 16000 and y.dtype == np.float32
            out.append(y)
            os.remove(str(name))
        assert out[0].shape == (5 * 80,) and out[1].shape == (6 * 80,)
        return out
    g1 = audio(['--top_p', '1e-6', '--temperature', '1', '--seed', '1'])
    g2 = audio(['--top_p', '1e-6', '--temperature', '1', '--seed', '2'])
    dflt = audio(['--seed', '1'])
    for a, b, d in zip(g1, g2, dflt):
        assert np.array_equal(a, b)
        assert not np.array_equal(a, d)


def test_opcheck_generate_ctrl_p_and_sample_rows(hip):
    import model as M
    from test_gpu_custom_ops import _model
    g = torch.Generator().manual_seed(2)
    m, _, c = _model(torch.float32, 't3')
    weights, meta = M.generation_weights(m)
    cond = torch.rand(2, 2, c['cond_dim'], generator=g).to(DEV)
    rb = M.top_row_bias(m, torch.tensor([1, 2], device=DEV))
    tau = torch.tensor([0.7, 1.0], device=DEV)
    k = torch.tensor([0, 5], dtype=torch.int32, device=DEV)
    p = torch.tensor([0.9, 1.0], device=DEV)
    torch.library.opcheck(torch.ops.srnn.generate_ctrl_p.default,
                          (weights, meta, cond, rb, None, 7, 0, 1, True, tau, k, p),
                          test_utils=('test_schema', 'test_faketensor'))
    z = torch.randn(2, 256, generator=g).to(DEV)
    q = torch.rand(2, 256, generator=g).to(DEV) + 0.1
    for args in ((z, q, 0, 0, 0, tau, k, p, True), (z, None, 5, 1, 2, None, None, p, False),
                 (z, None, 5, 0, 0, None, None, None, True)):
        torch.library.opcheck(torch.ops.srnn.sample_rows.default, args,
                              test_utils=('test_schema', 'test_faketensor'))


def test_new_symbols_are_exported(hip):
    import ctypes
    names = hip.exported_symbols()
    dll = ctypes.CDLL(hip.LIB_PATH)
    for sym in ('srnn_generate4', 'srnn_sample_rows', 'srnn_gen_persistent_rows_level'):
        assert sym in names
        assert getattr(dll, sym) is not None
    assert hip.gen_persistent_rows(torch.float32, 8, 64, 16, ctrl=True) == \
        hip.gen_persistent_rows(torch.float32, 8, 64, 16, ctrl=1)
    with pytest.raises(ValueError):
        hip.gen_persistent_rows(torch.float32, 8, 64, 16, ctrl=3)
