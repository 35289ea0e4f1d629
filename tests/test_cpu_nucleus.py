"""Nucleus (top-p) sampling without a GPU: model.nucleus_control, the host-side validation /
broadcasting of the control; the CPU reference of the draw (nucleus_ref.py) is honest -- with
p = 1 it IS sampling_ref.generate; and the condition the direct GPU tests rest on: every row of
the fixed synthetic set is far from its mass boundary and from a score tie."""
import numpy as np
import pytest
import torch

import nucleus_ref as N
import recipe
import sampling_ref as R


def test_nucleus_control_broadcast_and_none():
    import model as M
    assert M.nucleus_control(4) is None
    assert M.nucleus_control(4, 1.0) is None
    assert M.nucleus_control(3, [1.0, 1, 1]) is None
    assert M.nucleus_control(2, torch.ones(2)) is None
    assert M.nucleus_control(2, np.ones(2, dtype=np.float32)) is None
    p = M.nucleus_control(4, 0.9)
    assert p.dtype == torch.float32 and p.shape == (4,)
    assert p.tolist() == [float(np.float32(0.9))] * 4
    p = M.nucleus_control(3, [1.0, 0.5, 1e-6])
    assert p.tolist() == [1.0, 0.5, float(np.float32(1e-6))]
    p = M.nucleus_control(2, torch.tensor([0.25, 1.0], dtype=torch.float64))
    assert p.dtype == torch.float32 and p.tolist() == [0.25, 1.0]
    p = M.nucleus_control(2, np.array([1, 0.75]))
    assert p.tolist() == [1.0, 0.75]


@pytest.mark.parametrize('top_p', [
    0, 0.0, -0.1, 1.0001, 2, float('nan'), float('inf'), [0.5, 0.0], [0.5, float('nan')],
    [0.5, 0.5, 0.5], [0.5], [[0.5, 0.5]], 'most', 1e-60])
def test_nucleus_control_rejects(top_p):
    import model as M
    with pytest.raises(ValueError):
        M.nucleus_control(2, top_p)


def _fixed():
    import samplernn_oracle as O
    cfg = dict(recipe.CONFIGS['t3'], dim=64)
    orc = O.from_state_dict(cfg, recipe.make_weights(cfg, 7))
    B, n_cond = 8, 3
    cond = recipe.synth_cond((B, n_cond, cfg['cond_dim']), 4)
    spk = np.arange(B) % cfg['spk_dim']
    noise = torch.from_numpy(recipe.synth_noise((n_cond * 64, B, 256), 9))
    return orc, B, cond, spk, noise


def test_reference_with_p_off_is_the_top_k_reference():
    orc, B, cond, spk, noise = _fixed()
    tau, k = R.controls(B)
    want = R.generate(orc, B, cond, spk, noise, tau, k)
    got = N.generate(orc, B, cond, spk, noise, tau, k, [1.0] * B)
    for g, w in zip(got[:4], want):
        assert torch.equal(g, w)
    assert torch.isinf(got[4]).all()
    assert R.draw is not None and R.draw.__module__ == 'sampling_ref'   # (put back)


def test_reference_nucleus_on_fixed_inputs():
    """The reference with the loop tests' mixed controls, and the oracle-model near-boundary
    shares a model-level test would have to live with (printed, for orientation)."""
    orc, B, cond, spk, noise = _fixed()
    tau, k, p = N.controls(B)
    seq, lp, margin, kgap, gap = N.generate(orc, B, cond, spk, noise, tau, k, p)
    L = orc.lookback
    left, amb = N.check_self_consistent(lp, noise, seq, L, tau, k, p)
    assert left <= 0.01 * seq[:, L:].numel()
    # row 0 is at the defaults of all three: the oracle's own stream
    assert torch.equal(seq[0], orc.generate(B, cond, spk, noise)[0])
    # every draw lies in its row's nucleus, and the nucleus does bite
    lpt = lp.permute(1, 0, 2)
    inN, _, inS = N.nucleus(lpt, tau, k, p)
    x = seq[:, L:].t().unsqueeze(-1)
    assert bool(torch.gather(inN, -1, x).all())
    assert int(inN.sum()) < int(inS.sum())
    for pp in (0.9, 0.5):
        _, _, _, _, g = N.generate(orc, B, cond, spk, noise, [1.0] * B, [0] * B, [pp] * B)
        print('oracle model, p = %.2f, tau = 1: %.1f %% of steps within 1e-4 of the cut-off, '
              '%.1f %% within 1e-3' % (pp, 100 * float((g < 1e-4).float().mean()),
                                       100 * float((g < 1e-3).float().mean())))


def test_synthetic_rows_are_clear_of_their_boundaries():
    """The condition of the direct GPU tests (which compare indices exactly, no row left out):
    under the reference every row's boundary gap and score margin are >= 1e-3 -- ten times the
    device's allowed mass error -- and the set holds what it is meant to hold."""
    S = N.synthetic()
    print('boundary gap min %.4g, score margin min %.4g' % (float(S['gap'].min()),
                                                           float(S['margin'].min())))
    assert bool((S['gap'] >= 1e-3).all()), S['gap'].tolist()
    assert bool((S['margin'] >= 1e-3).all()), S['margin'].tolist()
    assert S['logits'].shape == (N.ROWS, 256) and S['noise'].shape == (N.ROWS, 256)
    sel = [b for b in range(N.ROWS) if S['tau'][b] > 0 and S['p'][b] < 1]
    for pp in N.PS[1:]:
        for tt in N.TAUS[:4]:
            for kk in N.KS:
                assert any(S['p'][b] == pp and S['tau'][b] == tt for b in sel), (pp, tt)
                assert any(S['p'][b] == pp and S['k'][b] == kk for b in sel), (pp, kk)
    # exact ties across the cut-off: the least probable logit of N is held by two classes
    for b in N.TIE_ROWS:
        z = S['logits'][b]
        assert b in sel and int((z == z[S['inN'][b]].min()).sum()) == 2
        assert bool(S['inN'][b][z == z[S['inN'][b]].min()].all())
    # rows where k cuts inside the would-be nucleus: N is all of S
    cut = [b for b in sel if S['k'][b] == 8 and bool((S['inN'][b] == S['inS'][b]).all())]
    assert len(cut) >= 2
    assert any(bool((S['logits'][b] == -100).any()) for b in N.TAIL_ROWS)
    # the adversarial noise: just inside N is drawn, just outside is not (and the draw stays in N)
    n_in = n_out = 0
    for b in sel:
        x, a = int(S['x'][b]), int(S['adv'][b])
        assert float(S['noise'][b, a]) == float(np.float32(1e-30))
        assert bool(S['inN'][b][x])
        if S['inside'][b]:
            assert bool(S['inN'][b][a]) and x == a
            n_in += 1
        else:
            assert not bool(S['inN'][b][a]) and x != a
            # without the nucleus that class would have been drawn
            free, _, _ = R.draw(S['logits'][b:b + 1], S['noise'][b:b + 1], [S['tau'][b]], [0])
            assert int(free[0]) == a
            n_out += 1
    assert n_in >= 16 and n_out >= 16
    # greedy rows ignore p and the noise
    for b in range(N.ROWS):
        if S['tau'][b] == 0:
            assert int(S['x'][b]) == int(S['logits'][b].argmax())
