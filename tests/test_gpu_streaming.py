"""Streamed generation on the device: carried state (Generator state= / return_state=, stream,
prime; srnn_generate5) and the forced prefix.

The contract: an utterance generated as consecutive calls, each continuing from the state the
previous one ended in, IS the one-shot utterance -- same indices, same log-probs, torch.equal
-- for both dtypes, the persistent and the per-sample path, device and replayed noise, every
fold variant, and from a graph-replayed block; a call forced along a stream reproduces it bit
for bit, and along a foreign stream reports the oracle's log-probs (stream_ref).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import recipe
import sampling_ref
import stream_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
L = 64
F32, BF16 = torch.float32, torch.bfloat16

# recipe.CONFIGS entries, dim raised to where the ticks fold: a multiple of 64 in fp32, and of
# 128 in bf16 (the GRU cell kernel that takes the folded ticks' precomputed gh needs whole
# 256-byte k stages; a bf16 model at dim 64 keeps the unfolded ticks)
CFGS = {
    't3': dict(recipe.CONFIGS['t3'], dim=64),          # fold + fold_top
    't3x128': dict(recipe.CONFIGS['t3'], dim=128),
    't4la': dict(recipe.CONFIGS['t4la'], dim=64),      # three tiers: fold without fold_top
    't4lax128': dict(recipe.CONFIGS['t4la'], dim=128),
    't3r2wn': recipe.CONFIGS['t3r2wn'],                # n_rnn = 2: unfolded, weight norm
    't2': recipe.CONFIGS['t2'],                        # a single tier
    'big': recipe.CONFIGS['big'],                      # D = 1024: the in-launch tick GEMM
}
_MODELS = {}


def build(name, dtype, seed=7):
    import model as M
    if dtype == BF16 and name in ('t3', 't4la'):
        name += 'x128'
    key = (name, dtype, seed)
    if key not in _MODELS:
        cfg = CFGS[name]
        m = M.SampleRNN(cfg['frame_sizes'], cfg['n_rnn'], cfg['dim'], cfg['learn_h0'],
                        cfg['q_levels'], True, cfg['weight_norm'], cfg['cond_dim'],
                        cfg['spk_dim'])
        m.compute_dtype = dtype
        M.Predictor(m).load_state_dict({k: torch.from_numpy(v.copy())
                                        for k, v in recipe.make_weights(cfg, seed).items()})
        _MODELS[key] = m.to(DEV)
    return _MODELS[key], CFGS[name]


def inputs(cfg, B, n_cond, seed=4):
    cond = recipe.synth_cond((B, n_cond, cfg['cond_dim']), seed)
    spk = np.arange(B) % cfg['spk_dim']
    noise = torch.from_numpy(recipe.synth_noise((n_cond * lookback(cfg), B, 256), seed + 5))
    return cond, spk, noise


def lookback(cfg):
    return int(np.prod(cfg['frame_sizes']))


def run(m, B, cond, spk, **kw):
    """One Generator call -> (indices of the generated steps (B, T), logp (B, T, Q), state)."""
    import model as M
    gen = M.Generator(m, True)
    want_state = kw.pop('return_state', True)
    res = gen(B, 0, cond, spk, return_logp=True, return_state=want_state, **kw)
    Lb = m.lookback
    return gen.last_sequences[:, Lb:].cpu(), res[1].cpu(), (res[2] if want_state else None)


def chunked(m, B, cond, spk, frames, noise=None, **kw):
    """The utterance as consecutive calls of `frames` conditioning frames each."""
    Lb = m.lookback
    state, seqs, lps, f0 = None, [], [], 0
    for n in frames:
        s, lp, state = run(m, B, cond[:, f0:f0 + n], spk, state=state,
                           noise=None if noise is None else noise[f0 * Lb:(f0 + n) * Lb], **kw)
        seqs.append(s)
        lps.append(lp)
        f0 += n
    assert f0 == cond.shape[1]
    return torch.cat(seqs, 1), torch.cat(lps, 1), state


def sampler_kw(sampler, noise):
    return dict(noise=noise) if sampler == 'noise' else dict(sampler='philox', seed=1234)


def assert_same(a, b):
    assert torch.equal(a[0], b[0]), 'indices differ at %s' % (a[0] != b[0]).nonzero()[:4].tolist()
    assert torch.equal(a[1], b[1]), 'log-probs differ, max %g' % (a[1] - b[1]).abs().max().item()


# ------------------------------------------------------------------ chunked == one-shot
@pytest.mark.parametrize('sampler', ['philox', 'noise'])
@pytest.mark.parametrize('persistent', [True, False])
@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('name', ['t3', 't4la', 't3r2wn', 't2'])
def test_chunked_equals_one_shot(hip, name, dtype, persistent, sampler):
    """n_cond = 6 as 2 + 1 + 3: the odd middle chunk ends with the top tier's h in buffer [1],
    the last runs a two-period block then a one-period one; B = 5 is a ragged row group."""
    m, cfg = build(name, dtype)
    B = 5
    if persistent:
        assert hip.gen_persistent_rows(dtype, B, cfg['dim'], 16) > 0
    cond, spk, noise = inputs(cfg, B, 6)
    kw = dict(sampler_kw(sampler, noise), persistent=persistent)
    one = run(m, B, cond, spk, **kw)
    parts = chunked(m, B, cond, spk, (2, 1, 3), **kw)
    assert_same(parts, one)
    assert torch.equal(parts[2].blob, one[2].blob)
    assert parts[2].steps.tolist() == [6 * m.lookback] * B


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_chunked_equals_one_shot_noise_in_loop(hip, monkeypatch, dtype):
    """SRNN_GEN_NOISE_AHEAD=0 moves the draw into the persistent loop; a continued Philox
    stream on the plain kernels still draws ahead (their own draw has no step origin), and the
    stream does not change either way."""
    m, cfg = build('t3', dtype)
    B = 5
    cond, spk, _ = inputs(cfg, B, 3)
    kw = dict(sampler='philox', seed=77)
    one = run(m, B, cond, spk, **kw)
    monkeypatch.setenv('SRNN_GEN_NOISE_AHEAD', '0')
    assert_same(run(m, B, cond, spk, **kw), one)
    assert_same(chunked(m, B, cond, spk, (1, 2), **kw), one)
    # (the controlled builds add the origin in the loop itself)
    forced = chunked(m, B, cond, spk, (1, 2), **kw)
    state = run(m, B, cond[:, :1], spk, **kw)[2]
    tail = run(m, B, cond[:, 1:], spk, state=state, prefix=one[0][:, L:],
               prefix_len=[0, 3, 64, 65, 128], **kw)
    assert torch.equal(tail[0], one[0][:, L:]) and torch.equal(tail[1], one[1][:, L:])
    assert torch.equal(forced[2].blob, tail[2].blob)


def test_chunked_equals_one_shot_bf16_d1024(hip):
    """D = 1024, bf16: the bottom tick's GEMM runs inside the persistent launch."""
    m, cfg = build('big', BF16, 11)
    B = 9
    assert hip.gen_persistent_rows(BF16, B, 1024, 16) > 0
    cond, spk, noise = inputs(cfg, B, 5)
    one = run(m, B, cond, spk, noise=noise)
    parts = chunked(m, B, cond, spk, (3, 2), noise=noise)
    assert_same(parts, one)
    assert torch.equal(parts[2].blob, one[2].blob)


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_chunked_equals_one_shot_graph(hip, dtype):
    """4 + 5 against 9 with graph replay: the second chunk's replayed graph runs from an
    imported state (and both one-shot and chunks without it give the same stream)."""
    m, cfg = build('t3', dtype)
    B = 5
    cond, spk, _ = inputs(cfg, B, 9)
    kw = dict(sampler='philox', seed=99)
    one = run(m, B, cond, spk, use_graph=True, **kw)
    assert_same(chunked(m, B, cond, spk, (4, 5), use_graph=True, **kw), one)
    assert_same(chunked(m, B, cond, spk, (4, 5), use_graph=False, **kw), one)


# ------------------------------------------------------------------ forced prefix
@pytest.mark.parametrize('persistent', [True, False])
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_self_forcing_reproduces_the_stream(hip, dtype, persistent):
    """A run forced along its own output for per-row lengths straddling the bottom tick (16) and
    the period (64) reproduces indices, log-probs and the end state bit for bit."""
    m, cfg = build('t3', dtype)
    B, n_cond = 9, 2
    T = n_cond * L
    if persistent:
        assert hip.gen_persistent_rows(dtype, B, cfg['dim'], 16, ctrl=True) > 0
    cond, spk, _ = inputs(cfg, B, n_cond)
    kw = dict(sampler='philox', seed=31, persistent=persistent)
    one = run(m, B, cond, spk, **kw)
    lens = [0, 1, 15, 16, 17, 63, 64, 65, T]
    forced = run(m, B, cond, spk, prefix=one[0], prefix_len=lens, **kw)
    assert_same(forced, one)
    assert torch.equal(forced[2].blob, one[2].blob)


@pytest.fixture(scope='module')
def foreign():
    """The oracle's run forced along a stream that is not its own (fp32, t3 at dim 64)."""
    import samplernn_oracle as O
    cfg = CFGS['t3']
    orc = O.from_state_dict(cfg, recipe.make_weights(cfg, 7))
    B, n_cond = 4, 2
    cond, spk, noise = inputs(cfg, B, n_cond, seed=21)
    rng = np.random.Generator(np.random.PCG64(77))
    prefix = torch.from_numpy(rng.integers(0, 256, (B, 100)))
    lens = [100, 37, 0, 64]
    seq, lp, margin, _ = stream_ref.generate(orc, B, cond, spk, noise, prefix=prefix, n_forced=lens)
    return dict(B=B, cond=cond, spk=spk, noise=noise, prefix=prefix, lens=lens, seq=seq, lp=lp,
                margin=margin)


def test_foreign_prefix_fp32(hip, foreign):
    """Forced positions hold the input, log-probs at every step are the oracle's within 1e-4
    (README "Parity": the fp32 log-prob bound), and the free draws after the prefix are the
    sampler definition's at tau = 1, k off.  On the CPU the oracle loop over these seeds leaves
    0 of its 311 free steps out (no margin below 1e-4; the smallest is 1.3e-3), far under
    check_self_consistent's cap, so the free draws must also be the oracle's own."""
    f = foreign
    m, _ = build('t3', F32)
    B = f['B']
    s, lp, _ = run(m, B, f['cond'], f['spk'], noise=f['noise'], prefix=f['prefix'],
                   prefix_len=f['lens'])
    for b, n in enumerate(f['lens']):
        assert torch.equal(s[b, :n], f['prefix'][b, :n])
    err = (lp - f['lp']).abs().max().item()
    print('foreign prefix: max |dlogp| vs the oracle %.3g' % err)
    assert err < 1e-4, err
    full = torch.cat([torch.full((B, L), 128, dtype=torch.long), s], 1)
    free = torch.arange(s.shape[1])[None, :] >= torch.tensor(f['lens'])[:, None]
    # forced steps are not draws: judged as draws they would fail, so their indices are
    # replaced by the definition's own before the check
    want = torch.argmax(lp.double() - torch.log(f['noise'].permute(1, 0, 2).double()), -1)
    judged = torch.where(free, s, want)
    n_out = sampling_ref.check_self_consistent(
        lp, f['noise'], torch.cat([full[:, :L], judged], 1), L, [1.0] * B, [0] * B)
    assert n_out <= 1
    assert torch.equal(s, f['seq'][:, L:])


# ------------------------------------------------------------------ rows of a state
@pytest.fixture(scope='module')
def two_chunks():
    """bf16 / fp32 one-shot runs over 3 frames and the state after the first 2, replayed noise."""
    out = {}
    for dtype in (F32, BF16):
        m, cfg = build('t3', dtype)
        B = 5
        cond, spk, noise = inputs(cfg, B, 3, seed=8)
        one = run(m, B, cond, spk, noise=noise)
        head = run(m, B, cond[:, :2], spk, noise=noise[:2 * L])
        out[dtype] = dict(m=m, B=B, cond=cond, spk=spk, noise=noise, one=one, head=head)
    return out


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_row_permutation(hip, two_chunks, dtype):
    r = two_chunks[dtype]
    perm = [3, 0, 4, 2, 1]
    s, lp, st = run(r['m'], r['B'], r['cond'][perm, 2:], r['spk'][perm],
                    noise=r['noise'][2 * L:, perm].contiguous(), state=r['head'][2].rows(perm))
    assert torch.equal(s, r['one'][0][perm, 2 * L:])
    assert torch.equal(lp, r['one'][1][perm, 2 * L:])
    assert torch.equal(st.blob, r['one'][2].blob[perm])


def test_row_subset_fp32(hip, two_chunks):
    """Rows [4, 1, 3] continue at B = 3.  Bit-identity across batch sizes is not promised (GEMM
    routing depends on the shape): the one-shot rows' samples are forced and the log-probs
    must agree within the fp32 bound."""
    r = two_chunks[F32]
    rows = [4, 1, 3]
    s, lp, st = run(r['m'], 3, r['cond'][rows, 2:], r['spk'][rows],
                    noise=r['noise'][2 * L:, rows].contiguous(), state=r['head'][2].rows(rows),
                    prefix=r['one'][0][rows, 2 * L:])
    assert torch.equal(s, r['one'][0][rows, 2 * L:])
    err = (lp - r['one'][1][rows, 2 * L:]).abs().max().item()
    print('subset continuation: max |dlogp| %.3g' % err)
    assert err < 1e-4, err
    assert st.steps.tolist() == [3 * L] * 3


def test_state_round_trip(hip, two_chunks, tmp_path):
    import model as M
    r = two_chunks[BF16]
    torch.save(r['head'][2].state_dict(), str(tmp_path / 's.pt'))
    d = torch.load(str(tmp_path / 's.pt'), weights_only=True)
    assert all(not v.is_cuda for v in d.values() if torch.is_tensor(v))
    back = M.GenState.from_state_dict(d, DEV)
    assert torch.equal(back.blob, r['head'][2].blob) and back.steps.tolist() == [2 * L] * r['B']
    for st in (back, r['head'][2].cpu()):               # (a host state is moved by the call)
        s, lp, _ = run(r['m'], r['B'], r['cond'][:, 2:], r['spk'], noise=r['noise'][2 * L:],
                       state=st)
        assert torch.equal(s, r['one'][0][:, 2 * L:]) and torch.equal(lp, r['one'][1][:, 2 * L:])


# ------------------------------------------------------------------ prime / stream
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_prime_then_free_run(hip, dtype):
    import model as M
    m, cfg = build('t3', dtype)
    B = 5
    cond, spk, _ = inputs(cfg, B, 3, seed=13)
    rng = np.random.Generator(np.random.PCG64(5))
    prefix = torch.from_numpy(rng.integers(0, 256, (B, 2 * L)))
    single = run(m, B, cond, spk, sampler='philox', seed=5, prefix=prefix)
    st = M.Generator(m, True).prime(prefix, cond[:, :2], spk, seed=5)
    assert st.steps.tolist() == [2 * L] * B
    s, lp, end = run(m, B, cond[:, 2:], spk, sampler='philox', seed=5, state=st)
    assert torch.equal(single[0][:, :2 * L], prefix)
    assert torch.equal(s, single[0][:, 2 * L:]) and torch.equal(lp, single[1][:, 2 * L:])
    assert torch.equal(end.blob, single[2].blob)


@pytest.mark.parametrize('sampler', ['torch', 'philox'])
def test_stream_equals_call(hip, sampler):
    import model as M
    m, cfg = build('t3', BF16)
    B = 5
    cond, spk, _ = inputs(cfg, B, 5, seed=17)
    gen = M.Generator(m, True)
    torch.manual_seed(4321)
    want = gen(B, 0, cond, spk, sampler=sampler, seed=8)
    torch.manual_seed(4321)
    blocks = list(gen.stream(B, cond, spk, 2, sampler=sampler, seed=8))
    assert [tuple(b.shape) for b in blocks] == [(B, 2 * L), (B, 2 * L), (B, L)]
    assert all(b.dtype == torch.float32 and not b.is_cuda for b in blocks)
    assert torch.equal(torch.cat(blocks, 1), want)
    assert gen.last_state.steps.tolist() == [5 * L] * B


# ------------------------------------------------------------------ rejections, defaults
def _raw_call(m, B, cond, spk, state_blob):
    """srnn_generate5 through ctypes on a caller-owned seq filled with a sentinel; returns
    (return code, message, seq)."""
    import model as M
    import samplernn_hip as H
    weights, meta = M.generation_weights(m)
    sm = M.srnn_model_struct(weights, meta)
    condt = torch.from_numpy(cond).to(DEV, torch.float32).contiguous()
    row_bias = M.top_row_bias(m, torch.from_numpy(spk).to(DEV))
    seq = torch.full((B, L + cond.shape[1] * L), 7, dtype=torch.long, device=DEV)
    sz = ctypes.c_size_t(0)
    H.lib().call('srnn_gen_workspace_size', ctypes.byref(sm), B, ctypes.byref(sz))
    ws = torch.empty(sz.value, device=DEV, dtype=torch.uint8)
    st = H.SrnnGenStream()
    st.state_in = H.ptr(state_blob)
    st.state_bytes = state_blob.numel()
    torch.cuda.synchronize()
    rc = H.lib().dll.srnn_generate5(ctypes.byref(sm), B, cond.shape[1], H.ptr(condt),
                                    H.ptr(row_bias), None, 3, 0, H.ptr(seq), None, H.ptr(ws),
                                    sz.value, 0, H.stream(), None, None, None, ctypes.byref(st))
    torch.cuda.synchronize()
    return rc, H.lib().dll.srnn_last_error().decode(), seq.cpu()


def test_foreign_states_are_rejected(hip, two_chunks, monkeypatch):
    r = two_chunks[BF16]
    m, B, cond, spk = r['m'], r['B'], r['cond'][:, 2:], r['spk']
    # the other dtype: same record size, another header
    m32, _ = build('t3x128', F32)
    _, _, other = run(m32, B, r['cond'][:, :2], spk, noise=r['noise'][:2 * L])
    assert other.blob.shape == r['head'][2].blob.shape
    with pytest.raises(RuntimeError, match='state row 0 has layout'):
        run(m, B, cond, spk, sampler='philox', state=other)
    rc, msg, seq = _raw_call(m, B, cond, spk, other.blob)
    assert rc == 1 and 'state row 0 has layout' in msg
    assert bool((seq == 7).all())                       # nothing was written, [0, L) included
    # another dim
    m48, cfg48 = build('t2', BF16)
    _, _, st48 = run(m48, B, *inputs(cfg48, B, 1)[:2], sampler='philox')
    with pytest.raises(RuntimeError, match='layout needs'):
        run(m, B, cond, spk, sampler='philox', state=st48)
    # taken with the folded ticks off, used with them on (and the top fold alone off: the same
    # size, another header)
    monkeypatch.setenv('SRNN_GEN_FOLD', '0')
    _, _, unfolded = run(m, B, r['cond'][:, :2], spk, noise=r['noise'][:2 * L])
    monkeypatch.delenv('SRNN_GEN_FOLD')
    assert unfolded.blob.shape[1] < r['head'][2].blob.shape[1]
    with pytest.raises(RuntimeError, match='layout needs'):
        run(m, B, cond, spk, sampler='philox', state=unfolded)
    rc, msg, seq = _raw_call(m, B, cond, spk, unfolded.blob)
    assert rc == 1 and bool((seq == 7).all())
    monkeypatch.setenv('SRNN_GEN_FOLD_TOP', '0')
    with pytest.raises(RuntimeError, match='state row 0 has layout'):
        run(m, B, cond, spk, sampler='philox', state=r['head'][2])
    monkeypatch.delenv('SRNN_GEN_FOLD_TOP')
    # and the state still continues the stream it came from
    s, _, _ = run(m, B, cond, spk, noise=r['noise'][2 * L:], state=r['head'][2])
    assert torch.equal(s, r['one'][0][:, 2 * L:])


def _op_args(m, B, cond, spk, noise, return_logp=True):
    import model as M
    weights, meta = M.generation_weights(m)
    condt = torch.from_numpy(cond).to(DEV, torch.float32).contiguous()
    row_bias = M.top_row_bias(m, torch.from_numpy(spk).to(DEV))
    return (weights, meta, condt, row_bias, noise.to(DEV), 11, 0, 1, return_logp)


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_defaults_are_the_plain_call(hip, dtype):
    """No state, prefix or controls: srnn::generate_stream is srnn::generate, bit for bit, on
    the plain plan (gen_persistent_rows(..., ctrl=False))."""
    m, cfg = build('t3', dtype)
    B = 5
    assert hip.gen_persistent_rows(dtype, B, cfg['dim'], 16, ctrl=False) > 0
    cond, spk, noise = inputs(cfg, B, 3)
    args = _op_args(m, B, cond, spk, noise)
    seq0, lp0 = torch.ops.srnn.generate(*args)
    seq1, lp1, st = torch.ops.srnn.generate_stream(*args, None, None, None, None, 0, None, None,
                                                   False)
    assert torch.equal(seq0, seq1) and torch.equal(lp0, lp1) and st.numel() == 0
    # philox at step0 = 0 as well
    pargs = args[:4] + (None,) + args[5:]
    seq2, _ = torch.ops.srnn.generate(*pargs)
    seq3, _, _ = torch.ops.srnn.generate_stream(*pargs, None, None, None, None, 0, None, None,
                                                False)
    assert torch.equal(seq2, seq3)
    with pytest.raises(ValueError, match='32-bit'):
        torch.ops.srnn.generate_stream(*pargs, None, None, None, None, 0xFFFFFFFF - 100, None,
                                       None, False)


def test_opcheck_generate_stream(hip):
    m, cfg = build('t3', BF16)
    B = 3
    cond, spk, noise = inputs(cfg, B, 1)
    args = _op_args(m, B, cond, spk, noise)
    _, _, st = torch.ops.srnn.generate_stream(*args, None, None, None, None, 0, None, None, True)
    prefix = torch.randint(0, 256, (B, 40), device=DEV)
    plen = torch.tensor([40, 0, 17], dtype=torch.int32, device=DEV)
    tau = torch.tensor([1.0, 0.7, 0.0], device=DEV)
    k = torch.tensor([0, 8, 0], dtype=torch.int32, device=DEV)
    utils = ('test_schema', 'test_faketensor')
    for extra in ((None, None, None, None, 0, None, None, True),
                  (tau, k, None, st, 64, prefix, plen, True),
                  (None, None, None, st, 0, prefix, None, False)):
        torch.library.opcheck(torch.ops.srnn.generate_stream.default, args + extra,
                              test_utils=utils)


# ------------------------------------------------------------------ CLI
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'jalil-saboorizadeh-multi-speaker-neural-vocoder_amd')


@pytest.mark.parametrize('mode', [['--sampler', 'torch'],
                                  ['--sampler', 'philox', '--batch_files', 'true']],
                         ids=['torch', 'philox-batch'])
def test_cli_chunk_frames(hip, tmp_path, mode):
    """generate.py --chunk_frames 2 writes the WAVs of the default run, byte for byte (a
    checkpoint of recipe weights and a 9 / 7-frame conditioning corpus; per file with the
    reference's sampler, and the batched path with the device sampler)."""
    import model as M
    from test_cpu_data import _write_corpus
    cfg = recipe.CONFIGS['t3_20_4']              # lookback 80 = the Ahocoder frame
    files = ['72e000', '75v000']
    _, cond = _write_corpus(str(tmp_path) + '/', files, frames=(9, 7))
    for s in ('72', '75'):                       # spk_dim = number of symlinks
        os.symlink(tmp_path, os.path.join(cond, 'spk' + s))
    (tmp_path / 'generate_cond_gina.list').write_text('\n'.join(files) + '\n')
    (tmp_path / 'generate_spk_gina.list').write_text('72\n75\n')
    os.makedirs(tmp_path / 'npy_datasets')
    np.save(str(tmp_path / 'npy_datasets' / 'spk_id.npy'), np.array(['72', '75']))
    mm = np.stack([np.full(43, -1e4), np.full(43, 1e4)])
    np.save(str(tmp_path / 'npy_datasets' / 'min_max_joint.npy'), mm)
    sd = {k: torch.from_numpy(v.copy())
          for k, v in recipe.make_weights(dict(cfg, spk_dim=2), 3).items()}
    exp = 'exp:S~frame_sizes:20,4~dim:32'
    os.makedirs(tmp_path / 'results' / exp / 'checkpoints')
    os.makedirs(tmp_path / 'results' / exp / 'samples')
    ck = 'results/%s/checkpoints/ep1-it1' % exp
    torch.save(sd, str(tmp_path / ck))
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))
    base = [sys.executable, '-u', os.path.join(PKG, 'generate.py'), '--model', ck,
            '--datasets_path', str(tmp_path) + '/', '--cond_set', 'cond/', '--frame_sizes', '20',
            '4', '--n_rnn', '2', '--dim', '32', '--learn_h0', 'false', '--n_samples', '2']
    got = []
    for extra in ([], ['--chunk_frames', '2']):
        r = subprocess.run(base + mode + extra, cwd=str(tmp_path), env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        wavs = {}
        for f, s in zip(files, ('72', '75')):
            name = tmp_path / 'results' / exp / 'samples' / ('ep1-it1_file-%s_spk-%s.wav'
                                                             % (f, s))
            wavs[f] = name.read_bytes()
            os.remove(str(name))
        got.append(wavs)
    assert got[0] == got[1]
    assert len(got[0][files[0]]) > 9 * 80 * 4
