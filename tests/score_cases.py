"""Reference, checker and defect list of the generation scores.  Not a test module.

A step's score pair (csrc/sampler.hpp row_score) is {log-prob of the step's sample, entropy of the
model's softmax in nats}.  The float64 reference is made from gen_cases.reference's own `logp`
and `seq`, which calls neither the product nor the CPU oracle:

    taken[b, t] = logp[b, t, seq[b, L + t]]          (the forced sample at a forced step)
    H[b, t]     = -sum_q exp(logp[b, t, q]) logp[b, t, q]

The checker's unit is gen_cases': (|got - ref| - ulp32(ref) / 2) / 2^-24.  The log-prob is held
to gen_cases.C_LSE (it is the dense log-prob, bit for bit), the entropy to C_ENT.

tests/test_gpu_scores.py runs the cases on the device; tests/test_cpu_score_cases.py shows, without
one, that the checker reports every defect of DEFECTS at the cap of 64 and that the stated
operation order in numpy fp32 (`fp32_scores`) stays inside the bound.
"""
import numpy as np

import gen_cases as G

# C_ENT: what the device's 256 expf terms, their products with d, the two wave sums, logf and the
# division may add to 0.5 ulp32 of the exact entropy, in units of 2^-24: the largest value over
# every case of test_gpu_scores.CASES on the MI355X, against the float64 reference, is 8.684 (the
# per-sample and the forced (16, 2) D = 64 cases, at entropies near 4.5 nats, where one ulp32 is 8
# units), doubled and rounded up -- the rule that set C_LSE.  The same operations
# in numpy fp32 (index-order sums) deviate by 3.77 units over test_cpu_score_cases' four cases.
C_ENT = 18
CAP = 64

DEFECTS = ('entropy_topk', 'entropy_tempered', 'forced_draw_logp', 'log2', 'transposed',
           'ragged_swapped')
TOPK, TAU = 5, 0.7


def lookback(ref):
    return ref.seq.shape[1] - ref.logp.shape[1]


def reference_scores(ref):
    """(B, T, 2) float64 from a gen_cases.reference run."""
    L = lookback(ref)
    x = ref.seq[:, L:]
    taken = np.take_along_axis(ref.logp, x[..., None], axis=-1)[..., 0]
    ent = -(np.exp(ref.logp) * ref.logp).sum(-1)
    return np.stack([taken, ent], axis=-1)


def fp32_scores(logits, x):
    """row_score's stated operations in numpy float32 (sums in index order, not the wave's tree):
    logits (..., 256), x (...) -> (..., 2) float32."""
    z = np.asarray(logits, dtype=np.float32)
    m = z.max(-1, keepdims=True)
    d = z - m
    e = np.exp(d)
    s = e.sum(-1, keepdims=True, dtype=np.float32)
    ls = np.log(s)
    u = (e * d).sum(-1, keepdims=True, dtype=np.float32)
    lp = np.take_along_axis(d, np.asarray(x)[..., None], axis=-1) - ls
    ent = np.maximum(np.float32(0), ls - u / s)
    return np.concatenate([lp, ent], axis=-1).astype(np.float32)


def units(got, want):
    """(|got - want| - ulp32(want) / 2) / 2^-24 per element."""
    got = np.asarray(got, dtype=np.float64)
    return (np.abs(got - want) - 0.5 * G.ulp32(want)) * 2.0 ** 24


def check_scores(scores, ref, c_ent=None, c_lse=None):
    """A (B, T, 2) device result against the reference run: shape, log-prob within c_lse, entropy
    within c_ent and never negative.  Returns the list of complaints, by (row, step)."""
    c_ent = C_ENT if c_ent is None else c_ent
    c_lse = G.C_LSE if c_lse is None else c_lse
    assert c_ent <= CAP, 'C_ENT above %d is refused' % CAP
    assert c_lse <= CAP, 'C_LSE above %d is refused' % CAP
    want = reference_scores(ref)
    got = np.asarray(scores, dtype=np.float64)
    if got.shape != want.shape:
        return ['scores: shape %s, reference %s' % (got.shape, want.shape)]
    out = []
    u = units(got, want)
    for k, name, c in ((0, 'log-prob', c_lse), (1, 'entropy', c_ent)):
        bad = ~(u[..., k] <= c)
        if bad.any():
            out += G._report(name, bad, got[..., k], want[..., k], ('row', 'step'))
    neg = got[..., 1] < 0
    if neg.any():
        out += G._report('negative entropy', neg, got[..., 1], want[..., 1], ('row', 'step'))
    return out


def defective(ref, noise, n_forced, defect):
    """The reference's scores with one of DEFECTS built in, as a float32 device result."""
    assert defect in DEFECTS, defect
    L = lookback(ref)
    B, T, _ = ref.logp.shape
    sc = reference_scores(ref)
    if defect == 'entropy_topk':
        # the entropy of the distribution renormalised over the TOPK largest logits
        kth = -np.partition(-ref.logits, TOPK - 1, axis=-1)[..., TOPK - 1:TOPK]
        z = np.where(ref.logits >= kth, ref.logits, -np.inf)
        m = z.max(-1, keepdims=True)
        lp = z - (m + np.log(np.exp(z - m).sum(-1, keepdims=True)))
        p = np.exp(lp)
        sc[..., 1] = -np.where(p > 0, p * np.where(p > 0, lp, 0.0), 0.0).sum(-1)
    elif defect == 'entropy_tempered':
        z = ref.logits / TAU
        m = z.max(-1, keepdims=True)
        lp = z - (m + np.log(np.exp(z - m).sum(-1, keepdims=True)))
        sc[..., 1] = -(np.exp(lp) * lp).sum(-1)
    elif defect == 'forced_draw_logp':
        assert n_forced is not None, 'a forced case is needed'
        draw = np.argmax(ref.logits - np.log(np.transpose(np.asarray(noise, np.float64),
                                                          (1, 0, 2))), -1)
        forced = ~G.forced_margin_mask(B, T, n_forced)
        x = np.where(forced, draw, ref.seq[:, L:])
        sc[..., 0] = np.take_along_axis(ref.logp, x[..., None], axis=-1)[..., 0]
    elif defect == 'log2':
        sc = sc / np.log(2.0)
    elif defect == 'transposed':
        # the (T, B, 2) device buffer read as (B, T, 2) without the permute
        sc = np.ascontiguousarray(np.transpose(sc, (1, 0, 2))).reshape(B, T, 2)
    elif defect == 'ragged_swapped':
        g0 = (B // 8) * 8
        assert B - g0 >= 2, 'a ragged group of at least two rows is needed'
        sc = np.concatenate([sc[:g0], sc[g0:][::-1]], axis=0)
    return sc.astype(np.float32)
