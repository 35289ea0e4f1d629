"""CPU reference of the nucleus (top-p) draw and the fixed synthetic rows of its direct tests,
shared by the nucleus tests.  Not a test module.

The definition (csrc/sampler.hpp, Generator's docstring) extends sampling_ref's: per row with
controls (tau, k, p), logits z and that step's noise q,
    S = sampling_ref's top-k set
    w_j = exp((z_j - max z) / tau) for j in S,  W = sum_S w_j
    N = {j in S : z_j >= v_p}, v_p the LARGEST logit value v with sum_{j in S, z_j >= v} w_j >= p W
        (the crossing class is in, ties at v_p are all kept); N = S when p = 1 or tau = 0
    x = argmax_{j in N} (z_j - tau log q_j), first index on ties; tau = 0: argmax_S z_j
Everything is evaluated in float64 from fp32 log-probs (or logits: only differences matter) and
the fp32 noise; p is taken as the float32 the device reads.

Boundary gap of a row: with the classes of S in order of falling probability, c_n the
normalised cumulative mass through the crossing class n (all of its ties included) and c_{n-1}
the mass above it,  gap = min(c_n - p, p - c_{n-1}).  It is how far the mass comparison is from
going the other way.  When the crossing class is the most probable one there is no smaller
nucleus to fall back to (the empty set never reaches p > 0), so the lower side does not exist
and gap = c_n - p.  Rows without a select (p = 1, tau = 0) have gap = inf.
"""
import numpy as np
import torch

import sampling_ref as R

# the loop tests' per-row nucleus masses, beside sampling_ref.TEMPERATURES / TOP_KS (row b of a
# larger batch takes entry b % 8; row 0 stays at the defaults of all three controls)
TOP_PS = [1.0, 0.9, 0.5, 0.95, 0.9, 0.5, 0.3, 0.99]


def controls(B):
    tau, k = R.controls(B)
    return tau, k, [TOP_PS[b % 8] for b in range(B)]


def _p64(p):
    return torch.as_tensor(np.asarray(p, dtype=np.float32)).double()


def nucleus(lp, tau, k, p):
    """lp (..., B, Q) fp32; tau, k, p (B,) -> (inN (..., B, Q) bool, gap (..., B) float64,
    inS (..., B, Q) bool)."""
    sc0, _ = R.scores(lp, torch.ones_like(lp), tau, k)     # log q = 0: lp inside S, -inf outside
    inS = ~torch.isneginf(sc0)
    lp64 = lp.double()
    tau = torch.as_tensor(tau, dtype=torch.float64)
    p = _p64(p)
    on = (tau > 0) & (p > 0) & (p < 1)                     # (B,)
    t = torch.where(on, tau, torch.ones_like(tau)).unsqueeze(-1)
    m = lp64.max(-1, keepdim=True).values
    w = torch.where(inS, torch.exp((lp64 - m) / t), torch.zeros_like(lp64))
    vals, idx = torch.sort(torch.where(inS, lp64, torch.full_like(lp64, -float('inf'))), dim=-1,
                           descending=True, stable=True)
    ws = torch.gather(w, -1, idx)
    cum = torch.cumsum(ws, -1)
    W = cum[..., -1:]
    excl = cum - ws
    new = torch.ones_like(vals, dtype=torch.bool)
    new[..., 1:] = vals[..., 1:] != vals[..., :-1]
    # mass strictly above a class's tie group (excl is non-decreasing and 0 at the first group)
    above = torch.cummax(torch.where(new, excl, torch.zeros_like(excl)), -1).values
    pw = p.unsqueeze(-1) * W
    ins = (above < pw) & ~torch.isneginf(vals)
    mass = (ws * ins).sum(-1)
    cross = torch.where(ins, above, torch.full_like(above, -1.0)).max(-1).values
    Wr = W.squeeze(-1)
    inf = torch.full_like(mass, float('inf'))
    lower = torch.where(cross > 0, p - cross / Wr, inf)    # (first group: no lower side)
    gap = torch.minimum(mass / Wr - p, lower)
    inN = torch.zeros_like(inS).scatter(-1, idx, ins)
    onx = on.expand(gap.shape)
    return torch.where(onx.unsqueeze(-1), inN, inS), torch.where(onx, gap, inf), inS


def draw(lp, q, tau, k, p):
    """The definition's index and its margins: (x (..., B) int64; margin (..., B): best minus
    second-best score in N, inf if N has one class; kgap as sampling_ref.scores; gap (..., B): the
    boundary gap)."""
    sc, kgap = R.scores(lp, q, tau, k)
    inN, gap, _ = nucleus(lp, tau, k, p)
    sc = torch.where(inN, sc, torch.full_like(sc, -float('inf')))
    top = torch.topk(sc, 2, dim=-1).values
    margin = top[..., 0] - top[..., 1]
    margin = torch.where(torch.isnan(margin), torch.full_like(margin, float('inf')), margin)
    return torch.argmax(sc, dim=-1), margin, kgap, gap


@torch.no_grad()
def generate(orc, n_seqs, cond, spk, noise, tau, k, p):
    """sampling_ref.generate's loop with this module's draw.  Returns (seq, logp (n, T, Q),
    margin (n, T), kgap (n, T), gap (n, T))."""
    gaps = []

    def draw3(lp, q, tau_, k_):
        x, margin, kgap, gap = draw(lp, q, tau_, k_, p)
        gaps.append(gap)
        return x, margin, kgap
    saved = R.draw
    R.draw = draw3
    try:
        seq, lp, margin, kgap = R.generate(orc, n_seqs, cond, spk, noise, tau, k)
    finally:
        R.draw = saved
    return seq, lp, margin, kgap, torch.stack(gaps, 1)


# ------------------------------------------------------------------ the synthetic rows
ROWS = 64
PS = [1.0, 0.5, 0.9, 0.95, 1e-6]
TAUS = [1.0, 0.7, 1.3, 0.5, 0.0]
KS = [0, 8, 255]
TAIL_ROWS = (7, 21, 38, 52)          # ranks >= 40 at -100
TIE_ROWS = (2, 8, 13, 27, 33, 44, 59)   # the crossing class and the next one share a logit
_SET = None


def synthetic():
    """The direct tests' 64 rows: dict of logits (64, 256) fp32, noise (64, 256) fp32, tau, k, p
    (lists), perm (rank -> class), inside (64,) bool: the adversarial class lies just inside N
    (else just outside; rows whose N is every class have it inside), adv (64,) the class given
    q = 1e-30, and the reference's x, margin, gap, inN, inS.

    Logits are the log of a geometric distribution of ratio 0.8 laid over a fixed random
    permutation of the classes, plus a per-row constant; row b takes p = PS[b % 5],
    tau = TAUS[(b // 5) % 5], k = KS[(b // 9) % 3]."""
    global _SET
    if _SET is not None:
        return _SET
    rng = np.random.RandomState(20240611)
    perm = rng.permutation(256)
    rank_lp = np.log(0.2) + np.arange(256) * np.log(0.8)
    z = np.empty((ROWS, 256), dtype=np.float64)
    z[:, perm] = rank_lp[None, :]
    z += rng.uniform(-8.0, 8.0, size=(ROWS, 1))
    for b in TAIL_ROWS:
        z[b, perm[40:]] = -100.0
    p = [PS[b % 5] for b in range(ROWS)]
    tau = [TAUS[(b // 5) % 5] for b in range(ROWS)]
    k = [KS[(b // 9) % 3] for b in range(ROWS)]
    z = torch.from_numpy(z.astype(np.float32))
    # exact ties across the cut-off: the class after the crossing one takes its logit
    permt = torch.from_numpy(perm)
    inN, _, _ = nucleus(z, tau, k, p)
    for b in TIE_ROWS:
        n = int(inN[b].sum())                       # ranks 0 .. n - 1 are in N
        assert 0 < n < 255
        z[b, permt[n]] = z[b, permt[n - 1]]
    inN, gap, inS = nucleus(z, tau, k, p)
    q = torch.from_numpy(rng.exponential(size=(ROWS, 256)).astype(np.float32)).clamp_min(1e-6)
    inside = torch.zeros(ROWS, dtype=torch.bool)
    adv = torch.full((ROWS,), -1, dtype=torch.long)
    neg = torch.full((256,), -float('inf'), dtype=torch.float64)
    for b in range(ROWS):
        zb = z[b].double()
        outside = torch.where(~inN[b], zb, neg)
        if b % 2 == 0 or not bool((~inN[b]).any()):
            # the least probable class of N (the crossing class; the last of its ties)
            cand = torch.where(inN[b], -zb, neg)
            j = int((cand == cand.max()).nonzero()[-1])
            inside[b] = True
        else:
            # the most probable class outside N (outside S where k cuts first)
            j = int(outside.argmax())
        adv[b] = j
        q[b, j] = 1e-30
    x, margin, _, gap = draw(z, q, tau, k, p)
    _SET = dict(logits=z, noise=q, tau=tau, k=k, p=p, perm=permt, inside=inside, adv=adv, x=x,
                margin=margin, gap=gap, inN=inN, inS=inS)
    return _SET


# ------------------------------------------------------------------ the loop's self-consistency
def check_self_consistent(lp, noise, seq, L, tau, k, p, eps=2e-4, cap=0.01):
    """Every drawn index is the float64 argmax, from the returned log-probs lp (B, T, Q) and
    the noise (T, B, Q), over {j in S : lp_j >= v} for a threshold v whose set lies between
    N(p - eps) and N(p + eps) (eps: twice the device's allowed mass error); where the boundary
    gap is >= eps that is exactly N(p).  As in sampling_ref.check_self_consistent a step is left
    out only if the score margin (in the set drawn from) or the k-th gap is below 1e-4; there the
    index must still be one of the two best of an admissible set.  At most `cap` of the steps may
    be left out.  Returns (left out, steps with more than one admissible set)."""
    lpt = lp.permute(1, 0, 2)                                  # (T, B, Q)
    sc, kgap = R.scores(lpt, noise, tau, k)
    p32 = _p64(p)
    on = (torch.as_tensor(tau, dtype=torch.float64) > 0) & (p32 < 1)
    # p - eps <= 0: the smallest nucleus, the top tie group (any tiny p gives it); p + eps >= 1:
    # all of S (p = 1 is "off" in nucleus(), which then returns S)
    plo = torch.where(on, (p32 - eps).clamp_min(1e-30), p32)
    phi = torch.where(on, (p32 + eps).clamp_max(1.0), p32)
    lo, _, inS = nucleus(lpt, tau, k, plo)
    hi, _, _ = nucleus(lpt, tau, k, phi)
    _, _, _, gap = draw(lpt, noise, tau, k, p)
    assert bool((lo <= hi).all())
    got = seq[:, L:].t()                                       # (T, B)
    ninf = torch.full_like(sc, -float('inf'))
    amb = (lo != hi).any(-1)                                   # (T, B)
    assert not bool((amb & (gap >= eps)).any())
    left = 0
    bad = []
    lp64 = lpt.double()
    # the common case at once: one admissible set, a clear margin, the index its argmax
    top = torch.topk(torch.where(lo, sc, ninf), 2, dim=-1)
    m0 = top.values[..., 0] - top.values[..., 1]
    m0 = torch.where(torch.isnan(m0), torch.full_like(m0, float('inf')), m0)
    clear = ~amb & (m0 >= 1e-4) & (kgap >= 1e-4) & (got == top.indices[..., 0])
    for t, b in (~clear).nonzero().tolist():
        if True:
            g = int(got[t, b])
            # the admissible sets: top sets of S (whole tie groups) from N(p - eps) to N(p + eps)
            sets = [lo[t, b]]
            if amb[t, b]:
                extra = (hi[t, b] & ~lo[t, b]).nonzero().flatten()
                for v in sorted(set(lp64[t, b, extra].tolist()), reverse=True):
                    sets.append(hi[t, b] & (lp64[t, b] >= v))
            ok = near = False
            for s in sets:
                top = torch.topk(torch.where(s, sc[t, b], ninf[t, b]), 2)
                margin = float(top.values[0] - top.values[1])
                margin = float('inf') if margin != margin else margin
                tight = margin < 1e-4 or float(kgap[t, b]) < 1e-4
                cand = set(top.indices.tolist())
                if float(kgap[t, b]) < 1e-4:
                    kb = int(torch.as_tensor(k)[b])
                    sc2, _ = R.scores(lpt[t, b:b + 1], noise[t, b:b + 1],
                                      [float(torch.as_tensor(tau)[b])], [kb + 1])
                    cand |= set(torch.topk(sc2[0], 2).indices.tolist())
                if g == int(top.indices[0]) and not tight:
                    ok = True
                    break
                if tight and g in cand:
                    near = True
            if ok:
                continue
            if near:
                left += 1
                continue
            bad.append('step %d row %d: loop %d (lp %.7g, score %.7g), N(p) argmax %d, gap %.3g, '
                       '%d admissible sets' % (t, b, g, lp64[t, b, g], sc[t, b, g],
                                               int(torch.where(lo[t, b], sc[t, b],
                                                               ninf[t, b]).argmax()),
                                               gap[t, b], len(sets)))
    print('nucleus draw: %d of %d steps left out (near-ties), %d steps with a boundary gap < %g'
          % (left, got.numel(), int(amb.sum()), eps))
    assert not bad, '%d of %d draws outside the definition: %s' % (len(bad), got.numel(),
                                                                   '; '.join(bad[:8]))
    assert left <= cap * got.numel(), 'too many steps left out: %d of %d' % (left, got.numel())
    return left, int(amb.sum())
