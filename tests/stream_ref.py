"""CPU reference of streamed generation, shared by the streaming tests.  Not a test module.

The oracle's generation loop as in sampling_ref.generate (through the oracle's public tier /
mlp), at the plain draw x = argmax(log p - log q) in float64, with two additions:

* a per-row forced prefix: at step t < n_forced[b] row b takes prefix[b, t] in place of the
  draw; its log-probs are still recorded;
* the recurrent state (hidden, history) = (per-tier hidden tensors, the last L sample
  indices) may be carried in and is returned, so an utterance can be cut into calls.
"""
import numpy as np
import torch


@torch.no_grad()
def generate(orc, n_seqs, cond, spk, noise, prefix=None, n_forced=None, state=None):
    """cond (n_seqs, F, C) or (F, C): the call's frames.  noise (T, n_seqs, Q), the call's own.
    prefix (n_seqs, P) int64 and n_forced (n_seqs,) (default P for every row).  state: None
    for a fresh start, else the (hidden, history) an earlier call returned.
    Returns (seq (n, L + T) int64, logp (n, T, Q), margin (n, T): best minus second-best
    score of the draw, state)."""
    import samplernn_oracle as O
    cond = torch.as_tensor(np.asarray(cond))
    if cond.dim() == 2:
        cond = cond.unsqueeze(0).expand(n_seqs, *cond.shape)
    spk = torch.as_tensor(np.asarray(spk)).reshape(-1).long()
    if spk.numel() == 1:
        spk = spk.expand(n_seqs)
    spk = spk.reshape(n_seqs, 1)
    noise = torch.as_tensor(np.asarray(noise))
    nt = len(orc.frame_sizes)
    L, Q, fs0 = orc.lookback, orc.q_levels, orc.frame_sizes[0]
    T = cond.shape[1] * L
    seq = torch.full((n_seqs, L + T), O.q_zero(Q), dtype=torch.long)
    if state is None:
        hidden = [None] * nt
    else:
        hidden = list(state[0])
        seq[:, :L] = state[1]
    if prefix is not None:
        prefix = torch.as_tensor(np.asarray(prefix)).long()
        nf = torch.full((n_seqs,), prefix.shape[1], dtype=torch.long) if n_forced is None \
            else torch.as_tensor(np.asarray(n_forced)).long()
    outs = [None] * nt
    lps, margins = [], []
    for i in range(L, L + T):
        for t in reversed(range(nt)):
            n = orc.nfs[t]
            if i % n != 0:
                continue
            prev = 2 * O.udequantize(seq[:, i - n: i], Q).unsqueeze(1)
            if t == nt - 1:
                j = i // L - 1
                out, h = orc.tier(t, prev, None, cond[:, j:j + 1], spk, hidden[t])
            else:
                fi = (i // n) % orc.frame_sizes[t + 1]
                out, h = orc.tier(t, prev, outs[t + 1][:, fi:fi + 1], None, None, hidden[t])
            hidden[t] = h
            outs[t] = out
        lp = orc.mlp(seq[:, i - fs0: i], outs[0][:, i % fs0: i % fs0 + 1])[:, 0]
        sc = lp.double() - torch.log(noise[i - L].double())
        top = torch.topk(sc, 2, dim=-1).values
        x = torch.argmax(sc, dim=-1)
        if prefix is not None and i - L < prefix.shape[1]:
            x = torch.where(i - L < nf, prefix[:, i - L], x)
        seq[:, i] = x
        lps.append(lp)
        margins.append(top[:, 0] - top[:, 1])
    return (seq, torch.stack(lps, 1), torch.stack(margins, 1),
            ([h.clone() for h in hidden], seq[:, -L:].clone()))


def state_rows(state, index):
    """Rows `index` of a (hidden, history) state (hidden tensors are (n_rnn, B, D))."""
    idx = torch.as_tensor(index, dtype=torch.long)
    return [h[:, idx] for h in state[0]], state[1][idx]
