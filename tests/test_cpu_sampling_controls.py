"""Sampling controls (temperature / top-k) without a GPU: the CPU reference of the controlled
draw (sampling_ref.py) is honest -- at the defaults it IS the oracle's generate -- and
model.sampling_controls, the host-side validation / broadcasting of the two controls."""
import numpy as np
import pytest
import torch

import recipe
import sampling_ref as R


def _oracle(cfg, seed):
    import samplernn_oracle as O
    return O.from_state_dict(cfg, recipe.make_weights(cfg, seed))


def test_reference_at_defaults_is_the_oracle():
    cfg = dict(recipe.CONFIGS['t3'], dim=64)
    orc = _oracle(cfg, 7)
    B, n_cond = 8, 3
    cond = recipe.synth_cond((B, n_cond, cfg['cond_dim']), 4)
    spk = np.arange(B) % cfg['spk_dim']
    noise = torch.from_numpy(recipe.synth_noise((n_cond * 64, B, 256), 9))
    want, wlp = orc.generate(B, cond, spk, noise, return_logp=True)
    got, lp, _, _ = R.generate(orc, B, cond, spk, noise, [1.0] * B, [0] * B)
    assert torch.equal(got, want)
    assert torch.equal(lp, wlp)
    # Q means "off" as 0 does
    got, _, _, _ = R.generate(orc, B, cond, spk, noise, [1.0] * B, [256] * B)
    assert torch.equal(got, want)


def test_reference_controls_on_fixed_inputs():
    """The controlled reference on the definition test's inputs: what the GPU test relies on
    (how many steps its 1e-4 / 1e-3 margins leave out), and the controls' visible effects."""
    cfg = dict(recipe.CONFIGS['t3'], dim=64)
    orc = _oracle(cfg, 7)
    B, n_cond = 8, 3
    cond = recipe.synth_cond((B, n_cond, cfg['cond_dim']), 4)
    spk = np.arange(B) % cfg['spk_dim']
    noise = torch.from_numpy(recipe.synth_noise((n_cond * 64, B, 256), 9))
    tau, k = R.controls(B)
    seq, lp, margin, kgap = R.generate(orc, B, cond, spk, noise, tau, k)
    L = orc.lookback
    assert R.check_self_consistent(lp, noise, seq, L, tau, k) <= 0.01 * B * n_cond * L
    full = ((margin >= 1e-3) & (kgap >= 1e-3)).all(1)
    assert int(full.sum()) >= 6
    x = seq[:, L:]
    # row 0 is at the defaults: the oracle's own stream, whatever the other rows do
    assert torch.equal(seq[0], orc.generate(B, cond, spk, noise)[0])
    # row 5 (k = 1) and row 6 (tau = 0) are greedy; row 3 stays inside its top 8
    assert torch.equal(x[5], lp[5].argmax(-1)) and torch.equal(x[6], lp[6].argmax(-1))
    rank = (lp[3] > torch.gather(lp[3], 1, x[3].unsqueeze(1))).sum(1)
    assert int(rank.max()) < 8


def test_sampling_controls_broadcast_and_none():
    import model as M
    assert M.sampling_controls(4, 1.0, 0) is None
    assert M.sampling_controls(4) is None
    assert M.sampling_controls(3, [1.0, 1, 1], np.array([0, 256, 0])) is None
    assert M.sampling_controls(2, torch.ones(2), torch.tensor([256, 256])) is None
    t, k = M.sampling_controls(4, 0.5, 0)
    assert t.dtype == torch.float32 and k.dtype == torch.int32
    assert t.tolist() == [0.5] * 4 and k.tolist() == [0] * 4
    t, k = M.sampling_controls(3, 1.0, 16)
    assert t.tolist() == [1.0] * 3 and k.tolist() == [16] * 3
    t, k = M.sampling_controls(3, [1.0, 0.0, 1.25], (0, 5, 256))
    assert t.tolist() == [1.0, 0.0, 1.25] and k.tolist() == [0, 5, 256]
    t, k = M.sampling_controls(2, np.array([0.7, 1.0], dtype=np.float32), torch.tensor([1, 0]))
    assert t.tolist() == [np.float32(0.7), 1.0] and k.tolist() == [1, 0]
    t, k = M.sampling_controls(2, 1, 3.0)             # an integral float is an integer
    assert k.tolist() == [3, 3] and k.dtype == torch.int32


@pytest.mark.parametrize('temperature,top_k', [
    (-0.5, 0), (float('nan'), 0), (float('inf'), 0), ([1.0, -1e-3], 0),
    (1.0, 2.5), (1.0, -1), (1.0, 257), (1.0, [0, 300]), (1.0, float('nan')),
    ([1.0, 1.0, 1.0], 0), (1.0, [1]), (1.0, [[1, 2]]), ('warm', 0)])
def test_sampling_controls_rejects(temperature, top_k):
    import model as M
    with pytest.raises(ValueError):
        M.sampling_controls(2, temperature, top_k)
