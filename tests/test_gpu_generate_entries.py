"""The C ABI's earlier generation entries (srnn_generate .. srnn_generate4), called directly.

Python reaches the library through srnn_generate5 alone (custom_ops._generate), so this is what
runs the four older entries: each must give the registered op's sequences and log-probs, bit for
bit -- they fill the same request record as srnn_generate5 does.
"""
import ctypes

import pytest
import torch

import recipe

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B, N_COND, SEED = 5, 3, 11


@pytest.fixture(scope='module')
def case(hip):
    """t3 at dim 64 in fp32, 5 rows, 3 conditioning frames (a two-period block and the odd one),
    replayed noise; per-row controls that switch each of tau, k and p on and off."""
    import model as M
    cfg = dict(recipe.CONFIGS['t3'], dim=64)
    m = M.SampleRNN(cfg['frame_sizes'], cfg['n_rnn'], cfg['dim'], cfg['learn_h0'],
                    cfg['q_levels'], True, cfg['weight_norm'], cfg['cond_dim'], cfg['spk_dim'])
    M.Predictor(m).load_state_dict({k: torch.from_numpy(v.copy())
                                    for k, v in recipe.make_weights(cfg, 7).items()})
    m = m.to(DEV)
    T = N_COND * m.lookback
    cond = torch.from_numpy(recipe.synth_cond((B, N_COND, cfg['cond_dim']), 4)).to(DEV)
    noise = torch.from_numpy(recipe.synth_noise((T, B, 256), 9)).to(DEV)
    weights, meta = M.generation_weights(m, torch.float32)
    row_bias = M.top_row_bias(m, (torch.arange(B) % cfg['spk_dim']).to(DEV))
    tau = torch.tensor([1.0, 0.7, 0.0, 1.3, 0.9], device=DEV)
    k = torch.tensor([0, 40, 3, 256, 17], dtype=torch.int32, device=DEV)
    p = torch.tensor([1.0, 0.9, 0.5, 0.8, 0.95], device=DEV)
    return dict(hip=hip, L=m.lookback, T=T, cond=cond, noise=noise, weights=weights, meta=meta,
                row_bias=row_bias, tau=tau, k=k, p=p,
                op_args=(weights, meta, cond, row_bias, noise, SEED, 0, 1, True))


def _entry(c, name, *controls):
    """(seq, logp) of one direct call of entry `name` with the case's inputs."""
    import model as M
    H = c['hip']
    ms = M.srnn_model_struct(c['weights'], c['meta'])
    seq = torch.full((B, c['L'] + c['T']), 128, dtype=torch.long, device=DEV)
    logp = torch.empty((c['T'], B, 256), device=DEV)
    sz = ctypes.c_size_t(0)
    H.lib().call('srnn_gen_workspace_size', ctypes.byref(ms), B, ctypes.byref(sz))
    ws = torch.empty(sz.value, dtype=torch.uint8, device=DEV)
    row0 = [] if name == 'srnn_generate' else [0]
    H.lib().call(name, ctypes.byref(ms), B, N_COND, H.ptr(c['cond']), H.ptr(c['row_bias']),
                 H.ptr(c['noise']), SEED, *row0, H.ptr(seq), H.ptr(logp), H.ptr(ws), sz.value, 1,
                 H.stream(), *[H.ptr(t) for t in controls])
    return seq, logp


def _same(got, want):
    assert torch.equal(got[0], want[0]), 'indices differ'
    assert torch.equal(got[1], want[1]), 'log-probs differ'


@pytest.mark.parametrize('name', ['srnn_generate', 'srnn_generate2'])
def test_plain_entries_equal_the_op(case, name):
    _same(_entry(case, name), torch.ops.srnn.generate(*case['op_args']))


def test_generate3_equals_generate_ctrl(case):
    want = torch.ops.srnn.generate_ctrl(*case['op_args'], case['tau'], case['k'])
    _same(_entry(case, 'srnn_generate3', case['tau'], case['k']), want)
    assert not torch.equal(want[0], torch.ops.srnn.generate(*case['op_args'])[0])


def test_generate4_equals_generate_ctrl_p(case):
    want = torch.ops.srnn.generate_ctrl_p(*case['op_args'], case['tau'], case['k'], case['p'])
    _same(_entry(case, 'srnn_generate4', case['tau'], case['k'], case['p']), want)
    assert not torch.equal(want[0], torch.ops.srnn.generate_ctrl(*case['op_args'], case['tau'],
                                                                 case['k'])[0])
