"""CPU reference of the controlled draw (temperature / top-k), shared by the sampling-control
tests.  Not a test module.

The definition (csrc/sampler.hpp, Generator's docstring), per row with controls (tau, k), logits
z and that step's noise q:
    S = {j : z_j >= v_k}, v_k the k-th largest z (ties kept); k = 0 or Q: every j
    tau > 0:  x = argmax_{j in S} (z_j - tau log q_j)        tau = 0:  x = argmax_{j in S} z_j
first index on ties.  Scores are evaluated in float64 from the fp32 log-probs (log_softmax(z):
a per-row shift of z, so the same order and argmax) and the fp32 noise.
"""
import numpy as np
import torch

# the fixed control pairs of the definition tests (row b of a larger batch takes pair b % 8)
TEMPERATURES = [1.0, 0.7, 1.3, 1.0, 0.5, 1.0, 0.0, 0.8]
TOP_KS = [0, 0, 0, 8, 16, 1, 0, 255]


def controls(B):
    return ([TEMPERATURES[b % 8] for b in range(B)], [TOP_KS[b % 8] for b in range(B)])


def scores(lp, q, tau, k):
    """lp, q (..., B, Q) fp32; tau, k (B,) -> (score (..., B, Q) float64, -inf outside S;
    kgap (..., B): k-th minus (k+1)-th largest log-prob, inf where top-k is off)."""
    lp = lp.double()
    Q = lp.shape[-1]
    tau = torch.as_tensor(tau, dtype=torch.float64)
    k = torch.as_tensor(k, dtype=torch.long)
    on = (k >= 1) & (k <= Q - 1)
    srt = torch.sort(lp, dim=-1, descending=True).values
    kk = torch.where(on, k, torch.ones_like(k))
    shape = lp.shape[:-1] + (1,)
    vk = torch.gather(srt, -1, (kk - 1).expand(lp.shape[:-1]).unsqueeze(-1))
    vk1 = torch.gather(srt, -1, kk.expand(lp.shape[:-1]).unsqueeze(-1))
    inf = torch.full(shape, float('inf'), dtype=torch.float64)
    onx = on.expand(lp.shape[:-1]).unsqueeze(-1)
    thr = torch.where(onx, vk, -inf)
    kgap = torch.where(onx, vk - vk1, inf).squeeze(-1)
    # (tau = 0: the noise is not used -- log q may be -inf and 0 * inf is nan)
    t = tau.unsqueeze(-1)
    noisy = lp - t * torch.log(q.double())
    sc = torch.where((t > 0).expand(lp.shape), noisy, lp)
    sc = torch.where(lp >= thr, sc, torch.full_like(sc, -float('inf')))
    return sc, kgap


def draw(lp, q, tau, k):
    """The definition's index and its margins: (x (..., B) int64, margin (..., B): best minus
    second-best allowed score (inf if one is allowed), kgap as in scores())."""
    sc, kgap = scores(lp, q, tau, k)
    top = torch.topk(sc, 2, dim=-1).values
    margin = top[..., 0] - top[..., 1]
    margin = torch.where(torch.isnan(margin), torch.full_like(margin, float('inf')), margin)
    return torch.argmax(sc, dim=-1), margin, kgap


@torch.no_grad()
def generate(orc, n_seqs, cond, spk, noise, tau, k):
    """OracleSampleRNN.generate's loop (through the oracle's public tier / mlp /
    reset_hidden_states) with the draw replaced by the definition.  Returns (seq (n, L + T)
    int64, logp (n, T, Q), margin (n, T), kgap (n, T))."""
    import samplernn_oracle as O
    cond = torch.as_tensor(np.asarray(cond))
    if cond.dim() == 2:
        cond = cond.unsqueeze(0).expand(n_seqs, *cond.shape)
    spk = torch.as_tensor(np.asarray(spk)).reshape(-1).long()
    if spk.numel() == 1:
        spk = spk.expand(n_seqs)
    spk = spk.reshape(n_seqs, 1)
    nt = len(orc.frame_sizes)
    L, Q, fs0 = orc.lookback, orc.q_levels, orc.frame_sizes[0]
    T = cond.shape[1] * L
    seq = torch.full((n_seqs, L + T), O.q_zero(Q), dtype=torch.long)
    orc.reset_hidden_states()
    outs = [None] * nt
    lps, margins, kgaps = [], [], []
    for i in range(L, L + T):
        for t in reversed(range(nt)):
            n = orc.nfs[t]
            if i % n != 0:
                continue
            prev = 2 * O.udequantize(seq[:, i - n: i], Q).unsqueeze(1)
            if t == nt - 1:
                j = i // L - 1
                out, h = orc.tier(t, prev, None, cond[:, j:j + 1], spk, orc.hidden[t])
            else:
                fi = (i // n) % orc.frame_sizes[t + 1]
                out, h = orc.tier(t, prev, outs[t + 1][:, fi:fi + 1], None, None, orc.hidden[t])
            orc.hidden[t] = h
            outs[t] = out
        lp = orc.mlp(seq[:, i - fs0: i], outs[0][:, i % fs0: i % fs0 + 1])[:, 0]
        x, m, g = draw(lp, noise[i - L], tau, k)
        seq[:, i] = x
        lps.append(lp)
        margins.append(m)
        kgaps.append(g)
    return seq, torch.stack(lps, 1), torch.stack(margins, 1), torch.stack(kgaps, 1)


def check_self_consistent(lp, noise, seq, L, tau, k, cap=0.01):
    """Every drawn index is the definition's argmax, computed in float64 from the returned
    log-probs lp (B, T, Q) and the noise (T, B, Q).  A step is left out only if the margin
    between the best and second-best allowed score, or between the k-th and (k+1)-th largest
    log-prob, is below 1e-4; there the drawn index must still be one of the two best candidates
    (with the allowed set taken either way at the k-th / (k+1)-th near-tie).  At most `cap` of
    the steps may be left out.  Returns the number left out."""
    lpt = lp.permute(1, 0, 2)                                  # (T, B, Q)
    sc, kgap = scores(lpt, noise, tau, k)
    want = torch.argmax(sc, dim=-1)
    top = torch.topk(sc, 2, dim=-1)
    margin = top.values[..., 0] - top.values[..., 1]
    margin = torch.where(torch.isnan(margin), torch.full_like(margin, float('inf')), margin)
    got = seq[:, L:].t()                                       # (T, B)
    out = (margin < 1e-4) | (kgap < 1e-4)
    n_out = int(out.sum())
    print('controlled draw: %d of %d steps left out (margin < 1e-4: %d, k-th gap < 1e-4: %d)'
          % (n_out, out.numel(), int((margin < 1e-4).sum()), int((kgap < 1e-4).sum())))
    bad = ((want != got) & ~out).nonzero()
    if bad.numel():
        info = ['step %d row %d: definition %d (score %.7g), loop %d (score %.7g), margin %.3g'
                % (t, b, want[t, b], sc[t, b, want[t, b]], got[t, b], sc[t, b, got[t, b]],
                   margin[t, b]) for t, b in bad[:8].tolist()]
        raise AssertionError('%d of %d draws differ from the definition: %s'
                             % (bad.shape[0], got.numel(), '; '.join(info)))
    for t, b in out.nonzero().tolist():
        cand = set(top.indices[t, b].tolist())
        kb = int(torch.as_tensor(k)[b])
        if kgap[t, b] < 1e-4:
            # the same draw with the (k+1)-th log-prob allowed too
            sc2, _ = scores(lpt[t, b:b + 1], noise[t, b:b + 1], [float(torch.as_tensor(tau)[b])],
                            [kb + 1])
            cand |= set(torch.topk(sc2[0], 2).indices.tolist())
        assert int(got[t, b]) in cand, (t, b, int(got[t, b]), sorted(cand))
    assert n_out <= cap * out.numel(), 'too many steps left out: %d of %d' % (n_out, out.numel())
    return n_out
