"""Per-row sampling controls (temperature / top-k) of the fused generation loop
(csrc/sampler.hpp sample_row_ctrl; Generator.__call__(temperature=, top_k=)).

* definition (fp32, replayed noise): every index drawn by the persistent loop and by the
  per-sample sampler kernel is the definition's argmax of the log-probs the loop reports; the
  default-controls row of a mixed batch is bit for bit its uncontrolled self; both paths agree;
  the streams are the CPU reference's (sampling_ref.py) up to its first near-tie;
* bf16 at the compiled D = 1024 shape, in-launch tick GEMM on and off, full and ragged groups;
* Philox noise: all-default arrays, greedy rows, and the drawn distribution;
* plumbing: rank-sharded generation, the generate.py flags, the registered op.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import recipe
import sampling_ref as R
from test_gpu_generation import build, generate

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), 'jalil-saboorizadeh-multi-speaker-neural-vocoder_amd')


# ------------------------------------------------------------------ definition, fp32
@pytest.fixture(scope='module')
def fixed(hip):
    """The definition test's fixed inputs, run once: controlled (both paths), uncontrolled,
    and the CPU reference."""
    import samplernn_oracle as O
    cfg = dict(recipe.CONFIGS['t3'], dim=64)
    m, _ = build(cfg, 7, torch.float32)
    B, n_cond = 8, 3
    assert hip.gen_persistent_rows(torch.float32, B, 64, 16, ctrl=True) > 0   # the controlled plan
    cond = recipe.synth_cond((B, n_cond, cfg['cond_dim']), 4)
    spk = np.arange(B) % cfg['spk_dim']
    noise = torch.from_numpy(recipe.synth_noise((192, B, 256), 9))
    tau, k = R.controls(B)
    out = {'noise': noise, 'tau': tau, 'k': k, 'L': m.lookback}
    for name, persistent in (('persistent', True), ('per_sample', False)):
        out[name] = generate(m, B, cond, spk, persistent, noise=noise, temperature=tau, top_k=k)
        out[name + '_plain'] = generate(m, B, cond, spk, persistent, noise=noise)
    orc = O.from_state_dict(cfg, recipe.make_weights(cfg, 7))
    out['cpu'] = R.generate(orc, B, cond, spk, noise, tau, k)
    return out


@pytest.mark.parametrize('path', ['persistent', 'per_sample'])
def test_draws_are_the_definition_fp32(fixed, path):
    seq, lp = fixed[path]
    R.check_self_consistent(lp, fixed['noise'], seq, fixed['L'], fixed['tau'], fixed['k'])


@pytest.mark.parametrize('path', ['persistent', 'per_sample'])
def test_default_row_is_its_uncontrolled_self(fixed, path):
    seq, lp = fixed[path]
    seq0, lp0 = fixed[path + '_plain']
    assert torch.equal(seq[0], seq0[0])
    assert torch.equal(lp[0], lp0[0])
    assert not torch.equal(seq, seq0)          # (the controls did change the other rows)


def test_paths_agree(fixed):
    s1, l1 = fixed['persistent']
    s0, l0 = fixed['per_sample']
    assert torch.equal(s1, s0)
    torch.testing.assert_close(l1, l0, atol=1e-4, rtol=0)


@pytest.mark.parametrize('path', ['persistent', 'per_sample'])
def test_streams_are_the_cpu_reference(fixed, path):
    seq, _ = fixed[path]
    cseq, _, margin, kgap = fixed['cpu']
    L = fixed['L']
    T = cseq.shape[1] - L
    near = (margin < 1e-3) | (kgap < 1e-3)                      # (B, T)
    cut = [int(near[b].nonzero()[0]) if near[b].any() else T for b in range(near.shape[0])]
    print('CPU reference: first near-tie step per row', cut)
    for b, c in enumerate(cut):
        assert torch.equal(seq[b, :L + c], cseq[b, :L + c]), (b, c)
    assert sum(c == T for c in cut) >= 6


# ------------------------------------------------------------------ bf16, D = 1024
@pytest.mark.parametrize('B,tg', [(128, '1'), (128, '0'), (9, '1'), (9, '0')])
def test_draws_are_the_definition_bf16_d1024(hip, monkeypatch, B, tg):
    monkeypatch.setenv('SRNN_GEN_TICK_GEMM', tg)
    cfg = recipe.CONFIGS['big']
    m, _ = build(cfg, 11, torch.bfloat16)
    assert hip.gen_persistent_rows(torch.bfloat16, B, 1024, 16, ctrl=True) > 0
    n_cond = 2
    cond = recipe.synth_cond((B, n_cond, cfg['cond_dim']), 5)
    spk = np.arange(B) % cfg['spk_dim']
    noise = torch.from_numpy(recipe.synth_noise((n_cond * 64, B, 256), 3))
    tau, k = R.controls(B)
    seq, lp = generate(m, B, cond, spk, True, noise=noise, temperature=tau, top_k=k)
    R.check_self_consistent(lp, noise, seq, m.lookback, tau, k)


@pytest.mark.parametrize('dtype,B,tg', [
    (torch.bfloat16, 128, '1'), (torch.bfloat16, 128, '0'), (torch.bfloat16, 9, '1'),
    (torch.bfloat16, 9, '0'), (torch.float32, 128, '1'), (torch.float32, 9, '1')])
def test_controlled_builds_at_defaults_are_the_plain_loop_d1024(hip, monkeypatch, dtype, B, tg):
    """The controlled builds change more than the draw (the next tick's gate operands are
    loaded after the sample loop; with the tick GEMM in the launch they are that launch's own
    output), so at D = 1024 -- the compiled bf16 shape with the in-launch tick GEMM on and off,
    and the fp32 build -- the controlled loop given all-default arrays must reproduce the plain
    loop bit for bit, index stream and log-probs, over 8 bottom ticks: any wrong or stale gate
    operand would change the hidden state and with it every later log-prob."""
    import model as M
    monkeypatch.setenv('SRNN_GEN_TICK_GEMM', tg)
    cfg = recipe.CONFIGS['big']
    m, _ = build(cfg, 11, dtype)
    assert hip.gen_persistent_rows(dtype, B, 1024, 16) > 0
    assert hip.gen_persistent_rows(dtype, B, 1024, 16, ctrl=True) > 0
    n_cond = 2
    cond = torch.from_numpy(recipe.synth_cond((B, n_cond, cfg['cond_dim']), 5)).to(
        DEV, torch.float32).contiguous()
    spk = torch.from_numpy(np.arange(B) % cfg['spk_dim']).to(DEV)
    noise = torch.from_numpy(recipe.synth_noise((n_cond * 64, B, 256), 3)).to(DEV)
    weights, meta = M.generation_weights(m)
    rb = M.top_row_bias(m, spk)
    args = (weights, meta, cond, rb, noise, 0, 0, 1, True)
    s0, l0 = torch.ops.srnn.generate(*args)
    s1, l1 = torch.ops.srnn.generate_ctrl(
        *args, torch.ones(B, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV))
    assert torch.equal(s1, s0)
    assert torch.equal(l1, l0)
    assert torch.isfinite(l0).all()


# ------------------------------------------------------------------ Philox
def _t3(seed=7):
    cfg = dict(recipe.CONFIGS['t3'], dim=64)
    m, _ = build(cfg, seed, torch.float32)
    return cfg, m


@pytest.mark.parametrize('persistent', [True, False])
def test_all_default_arrays_give_the_default_philox_stream(hip, persistent):
    """Explicit per-row arrays of default values take the plain path; the controlled kernels
    given all-default arrays (the op called directly) draw the same stream bit for bit."""
    import model as M
    cfg, m = _t3()
    B, n_cond = 8, 2
    cond = recipe.synth_cond((B, n_cond, cfg['cond_dim']), 4)
    spk = np.arange(B) % cfg['spk_dim']
    s0, l0 = generate(m, B, cond, spk, persistent, sampler='philox', seed=31)
    s1, l1 = generate(m, B, cond, spk, persistent, sampler='philox', seed=31,
                      temperature=[1.0] * B, top_k=np.zeros(B, dtype=np.int64))
    assert torch.equal(s1, s0) and torch.equal(l1, l0)
    weights, meta = M.generation_weights(m)
    condt = torch.from_numpy(cond).to(DEV, torch.float32).contiguous()
    rb = M.top_row_bias(m, torch.from_numpy(spk).to(DEV))
    s2, l2 = torch.ops.srnn.generate_ctrl(
        weights, meta, condt, rb, None, 31, 0, 1 | (0 if persistent else 2), True,
        torch.ones(B, device=DEV), torch.tensor([0, 256] * (B // 2), dtype=torch.int32, device=DEV))
    assert torch.equal(s2.cpu(), s0) and torch.equal(l2.permute(1, 0, 2).cpu(), l0)


@pytest.mark.parametrize('persistent', [True, False])
def test_temperature_zero_is_greedy(hip, persistent):
    cfg, m = _t3()
    B, n_cond = 8, 2
    cond = recipe.synth_cond((B, n_cond, cfg['cond_dim']), 4)
    spk = np.arange(B) % cfg['spk_dim']
    tau = [1.0, 0.0, 1.0, 0.0, 0.9, 1.0, 1.0, 0.0]
    seq, lp = generate(m, B, cond, spk, persistent, sampler='philox', seed=5, temperature=tau)
    L = m.lookback
    for b in (1, 3, 7):
        top = torch.topk(lp[b], 2, dim=-1)
        clear = (top.values[:, 0] - top.values[:, 1]) >= 1e-4
        assert clear.float().mean() > 0.5
        assert torch.equal(seq[b, L:][clear], top.indices[:, 0][clear])
    # greedy does not depend on the seed
    seq2, _ = generate(m, B, cond, spk, persistent, sampler='philox', seed=6, temperature=tau)
    for b in (1, 3, 7):
        assert torch.equal(seq2[b], seq[b])
    assert not torch.equal(seq2[0], seq[0])


def test_drawn_distribution(hip):
    """128 identical rows (one cond, one speaker), tau = 0.7, k = 4, seeds 0..7: the 1024
    draws of the first generated sample lie in the top 4 and follow the renormalised
    softmax(logp / tau) within 5 binomial sigma.  Philox is counter-based: a fixed outcome."""
    cfg, m = _t3()
    B = 128
    cond = recipe.synth_cond((1, cfg['cond_dim']), 4)
    tau, k = 0.7, 4
    draws, lp0 = [], None
    for seed in range(8):
        seq, lp = generate(m, B, cond, 2, True, sampler='philox', seed=seed, temperature=tau,
                           top_k=k)
        draws.append(seq[:, m.lookback])
        if lp0 is None:
            lp0 = lp[0, 0].double()
        torch.testing.assert_close(lp[:, 0], lp[:1, 0].expand(B, -1), atol=1e-5, rtol=0)
    draws = torch.cat(draws)
    top = torch.topk(lp0, k)
    assert top.values[-1] - torch.topk(lp0, k + 1).values[-1] > 1e-4
    p = torch.softmax(top.values / tau, 0)
    n = draws.numel()
    assert n == 1024
    counts = torch.stack([(draws == j).sum() for j in top.indices]).double()
    assert counts.sum() == n, 'draws outside the top %d' % k
    sigma = torch.sqrt(n * p * (1 - p))
    print('top-4 p', p.tolist(), 'counts', counts.tolist())
    assert ((counts - n * p).abs() <= 5 * sigma).all(), (counts.tolist(), (n * p).tolist())


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
        # rank 0's rows hold the only non-default top_k, rank 1's a greedy row
        tau = [1.0, 0.6, 1.0, 1.0, 0.0, 1.4]
        k = [0, 0, 12, 0, 0, 3]
        out = M.shard_generate(M.Generator(m, True), n, cond, spk, 99, sampler='philox',
                               temperature=tau, top_k=k)
        full = None
        if rank == 0:
            full = M.Generator(m, True)(n, 0, cond, spk, sampler='philox', seed=99,
                                        temperature=tau, top_k=k).numpy()
            plain = M.Generator(m, True)(n, 0, cond, spk, sampler='philox', seed=99).numpy()
            assert np.array_equal(full[0], plain[0]) and not np.array_equal(full[1:], plain[1:])
        q.put((rank, out.numpy(), full, None))
        D.barrier()
        import torch.distributed as dist
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, None, None, traceback.format_exc()))
        raise


def test_sharded_generation_with_controls_reproduces_single_process(hip):
    from test_gpu_distributed import _spawn
    got = _spawn(_shard_worker, ())
    full = got[0][1]
    for rank in (0, 1):
        assert np.array_equal(got[rank][0], full), rank


def _run(args, cwd):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-u'] + args, cwd=cwd, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_generate_cli_temperature(hip, tmp_path):
    """generate.py --temperature 0: the same audio whatever the --seed, and not the default
    run's.  A tiny untrained model saved as a checkpoint (no training run needed)."""
    import model as M
    from scipy.io import wavfile
    from test_cpu_data import _write_corpus
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
    g1 = audio(['--temperature', '0', '--seed', '1'])
    g2 = audio(['--temperature', '0', '--seed', '2'])
    dflt = audio(['--seed', '1'])
    for a, b, d in zip(g1, g2, dflt):
        assert np.array_equal(a, b)
        assert not np.array_equal(a, d)


def test_opcheck_generate_ctrl(hip):
    import model as M
    from test_gpu_custom_ops import _model
    g = torch.Generator().manual_seed(2)
    m, _, c = _model(torch.float32, 't3')
    weights, meta = M.generation_weights(m)
    cond = torch.rand(2, 2, c['cond_dim'], generator=g).to(DEV)
    rb = M.top_row_bias(m, torch.tensor([1, 2], device=DEV))
    tau = torch.tensor([0.7, 1.0], device=DEV)
    k = torch.tensor([0, 5], dtype=torch.int32, device=DEV)
    torch.library.opcheck(torch.ops.srnn.generate_ctrl.default,
                          (weights, meta, cond, rb, None, 7, 0, 1, True, tau, k),
                          test_utils=('test_schema', 'test_faketensor'))
