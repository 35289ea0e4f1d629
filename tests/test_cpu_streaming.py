"""Streamed generation, host side: the CPU reference the GPU tests compare against
(stream_ref), the validation of Generator's streaming arguments, GenState's bookkeeping, the
chunk-invariance of torch's exponential_ stream that Generator.stream('torch') rests on, and
the library's exports.  No GPU.
"""
import numpy as np
import pytest
import torch

import recipe
import stream_ref


def _oracle(cfg, seed=5):
    import samplernn_oracle as O
    return O.from_state_dict(cfg, recipe.make_weights(cfg, seed))


@pytest.fixture(scope='module')
def ref_run():
    """One one-shot oracle run shared by the reference's own tests."""
    cfg = recipe.CONFIGS['t3']
    orc = _oracle(cfg)
    B, n_cond = 3, 3
    cond = recipe.synth_cond((B, n_cond, cfg['cond_dim']), 4)
    spk = np.arange(B) % cfg['spk_dim']
    noise = torch.from_numpy(recipe.synth_noise((n_cond * 64, B, 256), 9))
    seq, lp, margin, state = stream_ref.generate(orc, B, cond, spk, noise)
    return dict(orc=orc, B=B, n_cond=n_cond, cond=cond, spk=spk, noise=noise, seq=seq, lp=lp,
                state=state)


def test_reference_matches_the_oracle(ref_run):
    r = ref_run
    want = r['orc'].generate(r['B'], r['cond'], r['spk'], r['noise'])
    assert torch.equal(r['seq'], want)


def test_reference_chunked_equals_one_shot(ref_run):
    r = ref_run
    L = 64
    state, seqs, lps = None, [], []
    f0 = 0
    for n in (1, 2):
        s, lp, _, state = stream_ref.generate(r['orc'], r['B'], r['cond'][:, f0:f0 + n], r['spk'],
                                              r['noise'][f0 * L:(f0 + n) * L], state=state)
        seqs.append(s[:, L:])
        lps.append(lp)
        f0 += n
    assert torch.equal(torch.cat(seqs, 1), r['seq'][:, L:])
    assert torch.equal(torch.cat(lps, 1), r['lp'])
    assert all(torch.equal(a, b) for a, b in zip(state[0], r['state'][0]))
    assert torch.equal(state[1], r['state'][1])


def test_reference_self_forcing_reproduces_the_stream(ref_run):
    r = ref_run
    L = 64
    nf = [0, 17, r['n_cond'] * L]
    # (other noise: a forced step must not depend on it, a free step of row 0 does)
    s, lp, _, _ = stream_ref.generate(r['orc'], r['B'], r['cond'], r['spk'], r['noise'],
                                      prefix=r['seq'][:, L:], n_forced=nf)
    assert torch.equal(s, r['seq']) and torch.equal(lp, r['lp'])
    other = torch.from_numpy(recipe.synth_noise(tuple(r['noise'].shape), 10))
    s2, lp2, _, _ = stream_ref.generate(r['orc'], r['B'], r['cond'], r['spk'], other,
                                        prefix=r['seq'][:, L:], n_forced=nf)
    assert torch.equal(s2[2], r['seq'][2]) and torch.equal(lp2[2], r['lp'][2])
    assert torch.equal(s2[1, :L + 17], r['seq'][1, :L + 17])
    assert not torch.equal(s2[0], r['seq'][0])


@pytest.mark.parametrize('shape,cuts', [((384, 5, 256), (64, 192)), ((4096, 16, 256), (1, 1031))])
def test_exponential_stream_is_chunk_invariant(shape, cuts):
    """torch.empty(T, n, Q).exponential_() equals the concatenation of the draws of its chunks
    under the same seed: Generator.stream(sampler='torch') draws each chunk's noise separately
    and must still replay the one-shot stream."""
    torch.manual_seed(1234)
    whole = torch.empty(*shape).exponential_(1)
    torch.manual_seed(1234)
    T = shape[0]
    edges = (0,) + cuts + (T,)
    parts = [torch.empty(b - a, *shape[1:]).exponential_(1) for a, b in zip(edges, edges[1:])]
    assert torch.equal(torch.cat(parts), whole)


def _model(cfg):
    import model as M
    return M.SampleRNN(cfg['frame_sizes'], cfg['n_rnn'], cfg['dim'], cfg['learn_h0'],
                       cfg['q_levels'], True, cfg['weight_norm'], cfg['cond_dim'], cfg['spk_dim'])


def test_forced_prefix_validation():
    import model as M
    m = _model(recipe.CONFIGS['t3'])
    n, T = 3, 128
    idx = torch.randint(0, 256, (n, 100))
    p, pl = M.forced_prefix(m, n, T, idx, None)
    assert torch.equal(p, idx) and pl is None
    p, pl = M.forced_prefix(m, n, T, idx, 7)
    assert pl.dtype == torch.int32 and pl.tolist() == [7, 7, 7]
    p, pl = M.forced_prefix(m, n, T, idx, [0, 100, 5])
    assert pl.tolist() == [0, 100, 5]
    assert M.forced_prefix(m, n, T, None, None) == (None, None)
    # a float waveform is quantised with the model's quantiser
    import utils
    wave = torch.linspace(-1, 1, 100).repeat(n, 1)
    p, _ = M.forced_prefix(m, n, T, wave, None)
    assert torch.equal(p, utils.uquantize(wave, 256).clamp(max=255)) and int(p.max()) == 255
    for bad_len in (-1, 101, [0, 1], [[1, 2, 3]], 1.5, [0, 1, 101]):
        with pytest.raises(ValueError):
            M.forced_prefix(m, n, T, idx, bad_len)
    with pytest.raises(ValueError):
        M.forced_prefix(m, n, T, None, 3)                       # a length without a prefix
    with pytest.raises(ValueError):
        M.forced_prefix(m, n, T, torch.zeros(n, T + 1, dtype=torch.long), None)   # too wide
    with pytest.raises(ValueError):
        M.forced_prefix(m, n, T, torch.zeros(n + 1, 4, dtype=torch.long), None)   # rows
    with pytest.raises(ValueError):
        M.forced_prefix(m, n, T, torch.full((n, 4), 256), None)                   # index range
    with pytest.raises(ValueError):
        M.forced_prefix(m, n, T, torch.full((n, 4), -1), None)


def test_prime_length_mismatch():
    import model as M
    m = _model(recipe.CONFIGS['t3'])
    gen = M.Generator(m)
    cond = np.zeros((2, 43), dtype=np.float32)                  # 2 frames: 128 samples
    for width in (127, 129, 64):
        with pytest.raises(ValueError, match='num_cond'):
            gen.prime(torch.zeros(3, width, dtype=torch.long), cond, 0)


def _state(n=5, row_bytes=24, steps=None):
    import model as M
    blob = torch.arange(n * row_bytes, dtype=torch.int64).remainder(251).to(torch.uint8)
    return M.GenState(blob.reshape(n, row_bytes), [0, 2, 1, 64, 64, row_bytes],
                      steps if steps is not None else torch.arange(n) * 64)


def test_gen_state_rows_and_round_trip(tmp_path):
    import model as M
    st = _state()
    sub = st.rows([4, 1, 3])
    assert sub.n_seqs == 3 and sub.layout == st.layout
    assert torch.equal(sub.blob, st.blob[[4, 1, 3]]) and sub.steps.tolist() == [256, 64, 192]
    fork = st.rows(torch.tensor([2, 2]))
    assert torch.equal(fork.blob[0], fork.blob[1]) and fork.steps.tolist() == [128, 128]
    for bad in ([5], [-1], []):
        with pytest.raises(IndexError):
            st.rows(bad)
    d = st.state_dict()
    assert set(d) == {'blob', 'steps', 'layout'}
    torch.save(d, str(tmp_path / 'state.pt'))
    back = M.GenState.from_state_dict(torch.load(str(tmp_path / 'state.pt'), weights_only=True))
    assert torch.equal(back.blob, st.blob) and torch.equal(back.steps, st.steps)
    assert back.layout == st.layout and back.cpu().device.type == 'cpu'
    with pytest.raises(ValueError):
        M.GenState(st.blob, st.layout, torch.zeros(4))          # one step count per row
    with pytest.raises(ValueError):
        M.GenState(st.blob.reshape(-1), st.layout, st.steps)


def test_mixed_step_counts_need_replayed_noise():
    import model as M
    st = _state()
    with pytest.raises(ValueError, match='differing step counts'):
        M.Generator._stream_state(st, 5, 'cpu', True)
    blob, step0 = M.Generator._stream_state(st, 5, 'cpu', False)          # replayed noise
    assert step0 == 0 and torch.equal(blob, st.blob)
    even = _state(steps=torch.full((5,), 192))
    assert M.Generator._stream_state(even, 5, 'cpu', True)[1] == 192
    with pytest.raises(ValueError, match='rows'):
        M.Generator._stream_state(even, 4, 'cpu', True)
    with pytest.raises(TypeError):
        M.Generator._stream_state(even.blob, 5, 'cpu', True)
    assert M.Generator._stream_state(None, 5, 'cpu', True) == (None, 0)


def test_library_exports_the_streaming_entry_points():
    import ctypes
    import samplernn_hip as H
    dll = ctypes.CDLL(H.LIB_PATH)
    for name in ('srnn_generate5', 'srnn_gen_state_bytes'):
        assert hasattr(dll, name), name
        assert name in H._SIGS and name in H.exported_symbols()
    assert dll.srnn_abi_version() == 2
    # the state size: a multiple of the row count, 0 on bad arguments; a folded model carries
    # the two 3 D gh rows an unfolded one does not, and the ticks fold where the GRU cell takes
    # the carried gh: dim a multiple of 128 in bf16, of 64 in fp32
    import custom_ops
    for D, dt, fold in ((128, H.BF16, True), (128, H.F32, True), (64, H.F32, True),
                        (64, H.BF16, False), (48, H.BF16, False), (48, H.F32, False)):
        meta = [2, 1, D, 256, 43, dt, 16, 16, 16, 1, 4, 64, 107, 0, 64]
        plain = 4 * (16 + 64 + 2 * D)
        assert custom_ops.gen_state_row_bytes(meta) == plain + (4 * 6 * D if fold else 0), (D, dt)
    dll.srnn_gen_state_bytes.restype = ctypes.c_size_t
    dll.srnn_gen_state_bytes.argtypes = [ctypes.c_void_p, ctypes.c_int]
    m = H.SrnnModel()
    assert dll.srnn_gen_state_bytes(ctypes.byref(m), 4) == 0          # n_tiers 0
    assert dll.srnn_gen_state_bytes(None, 4) == 0
