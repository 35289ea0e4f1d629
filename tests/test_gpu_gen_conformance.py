"""Exact conformance sweep for the generation kernels (csrc/generate.hip, gen_mlp.hip,
gen_rows.hip) against gen_cases.reference, a float64 restatement that calls neither the product
nor the CPU oracle.

Method A (TABLE_A, CARRY): integer models whose whole index stream, final h, carried gh and
history are known bit for bit whatever the dtype, the association and the path; log-probs within
0.5 ulp32 + C_LSE 2^-24 of the float64 log-softmax of the exact logits.  Each row names the model,
the width, the dtype, (B, n_cond), the control level, graph / eager, the per-sample path, the
forced prefix and the one switch that is off; the record's fold bits and
gen_persistent_rows(...) > 0 must be what gen_cases.route restates for the row.
Method T (TABLE_T): teacher-forced random-weight models, every step compared: fp32 within 4 x the
CPU fp32 oracle's own deviation from the reference, bf16 within 2 x the deviation the rounding
points cause in the reference (max and mean).
tests/test_cpu_gen_cases.py proves every method A case exact by itself, that the tables reach both
sides of every route condition, and that the checkers report the listed defects by element.
"""
import numpy as np
import pytest
import torch

import gen_cases as G

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TD = {'fp32': torch.float32, 'bf16': torch.bfloat16}
_models = {}


def device_model(model, dtype, tag):
    """The product model of a (cfg, state dict) on the device (the last few are kept)."""
    import model as M
    cfg, sd = model
    key = (G._key(cfg), tag, dtype)
    if key not in _models:
        while len(_models) >= 4:
            _models.pop(next(iter(_models)))
        m = M.SampleRNN(cfg['frame_sizes'], cfg['n_rnn'], cfg['dim'], cfg['learn_h0'],
                        cfg['q_levels'], True, cfg['weight_norm'], cfg['cond_dim'], cfg['spk_dim'])
        m.compute_dtype = TD[dtype]
        M.Predictor(m).load_state_dict({k: torch.from_numpy(v.copy())
                                        for k, v in G.state_dict_f32(sd).items()})
        _models[key] = m.to(DEV)
    return _models[key]


def call(m, c, cond, spk, noise, prefix=None, n_forced=None, state=None, return_state=True):
    import model as M
    gen = M.Generator(m, True)
    kw = {}
    if prefix is not None:
        kw = dict(prefix=torch.from_numpy(prefix), prefix_len=torch.from_numpy(n_forced))
    res = gen(c.B, 0, cond, spk, noise=torch.from_numpy(noise), return_logp=True,
              use_graph=c.graph, persistent=c.persistent, controls_level=c.level, state=state,
              return_state=return_state, **kw)
    torch.cuda.synchronize()
    return (gen.last_sequences.cpu().numpy(), res[1].cpu().numpy(),
            res[2] if return_state else None)


def check_route(hip, c, r):
    rows = hip.gen_persistent_rows(TD[c.dtype], c.B, c.D, c.fs[0], ctrl=c.level)
    assert (rows > 0) == (r.form is not None), \
        '%s: gen_persistent_rows %d, the table names %r' % (c.id, rows, r.form)


def fail_if(c, msgs):
    assert not msgs, '%s: %s' % (c.id, ' | '.join(msgs))


@pytest.mark.parametrize('c', G.table_a(), ids=lambda c: c.id)
def test_method_a(hip, monkeypatch, c):
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    model, cond, spk, noise, prefix, n_forced, ref = G.inputs(c)
    m = device_model(model, c.dtype, 'int')
    r = G.route(c.cfg, c.dtype, c.B, c.env, c.persistent)
    check_route(hip, c, r)
    bits = (1 if r.fold else 0) | (2 if r.fold_top else 0)
    seq, lp, st = call(m, c, cond, spk, noise, prefix, n_forced)
    print('%s C_LSE units %.3f' % (c.id, G.logp_units(lp, ref).max()))
    rec = G.parse_state(st.blob.cpu().numpy(), c.cfg, r.fold)
    fail_if(c, G.check_case(seq, lp, rec, ref, c.cfg, c.dtype, bits, G.C_LSE))
    assert st.steps.tolist() == [ref.state['steps']] * c.B
    if prefix is None:
        # the plain entry (srnn::generate / generate_ctrl / generate_ctrl_p): the same stream
        seq2, lp2, _ = call(m, c, cond, spk, noise, return_state=False)
        fail_if(c, G.check_case(seq2, lp2, None, ref, c.cfg, c.dtype, bits, G.C_LSE))


@pytest.mark.parametrize('c', G.CARRY, ids=lambda c: c.id)
def test_state_carry(hip, c):
    """One call, calls over n_cond splits 1 | 2 | 2 and a session's chunks: every part and every
    record against the reference's own parts."""
    import model as M
    model, cond, spk, noise, _, _, ref = G.inputs(c)
    m = device_model(model, c.dtype, 'int')
    r = G.route(c.cfg, c.dtype, c.B, c.env, c.persistent)
    bits = (1 if r.fold else 0) | (2 if r.fold_top else 0)
    L = int(np.prod(c.fs))
    # (the parts of the one run: test_cpu shows that calls chained through the reference's own
    #  state give exactly these)
    parts, f0 = [], 0
    for n in G.SPLITS:
        parts.append((f0, n, G.part(ref, c.cfg, f0, n)))
        f0 += n
    # one call
    seq, lp, st = call(m, c, cond, spk, noise)
    rec = G.parse_state(st.blob.cpu().numpy(), c.cfg, r.fold)
    fail_if(c, ['one call: %s' % s
                for s in G.check_case(seq, lp, rec, ref, c.cfg, c.dtype, bits, G.C_LSE)])
    # calls over the splits
    st = None
    for f0, n, rp in parts:
        seq, lp, st = call(m, c, cond[:, f0:f0 + n], spk, noise[f0 * L:(f0 + n) * L], state=st)
        rec = G.parse_state(st.blob.cpu().numpy(), c.cfg, r.fold)
        fail_if(c, ['frames [%d, %d): %s' % (f0, f0 + n, s)
                    for s in G.check_case(seq, lp, rec, rp, c.cfg, c.dtype, bits, G.C_LSE)])
    # a session's chunks
    gen = M.Generator(m, True)
    with gen.session(c.B, max(G.SPLITS), return_logp=True, replay_noise=True) as ses:
        for f0, n, rp in parts:
            _, lp = ses.chunk(cond[:, f0:f0 + n], spk if f0 == 0 else None,
                              noise=torch.from_numpy(noise[f0 * L:(f0 + n) * L]))
            seq = np.concatenate([rp.seq[:, :L], ses.last_sequences.cpu().numpy()], axis=1)
            rec = G.parse_state(ses.state().blob.cpu().numpy(), c.cfg, r.fold)
            fail_if(c, ['session frames [%d, %d): %s' % (f0, f0 + n, s)
                        for s in G.check_case(seq, lp.cpu().numpy(), rec, rp, c.cfg, c.dtype, bits,
                                              G.C_LSE)])


@pytest.mark.parametrize('c', G.TABLE_T, ids=lambda c: c.id)
def test_method_t(hip, monkeypatch, c):
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    model, cond, spk, noise, prefix, ref, bound = G.inputs_t(c)
    m = device_model(model, c.dtype, 'rnd%d' % c.seed)
    r = G.route(c.cfg, c.dtype, c.B, c.env, c.persistent)
    seq, lp, st = call(m, c, cond, spk, noise, prefix, np.full(c.B, prefix.shape[1], np.int32))
    assert np.array_equal(seq, ref.seq), 'the forced stream was not followed'
    # the record's fold bits: the route the device took is the association the bound was made in
    word6 = st.blob.cpu().numpy().view(np.uint32)[:, 6]
    want = {'unfolded': 0, 'folded': 1, 'folded_top': 3}[c.assoc]
    assert (word6 == want).all(), '%s: fold bits %s, the case names %s' % (c.id, word6[:4], c.assoc)
    rec = G.parse_state(st.blob.cpu().numpy(), c.cfg, r.fold)
    err = np.abs(lp.astype(np.float64) - ref.logp)
    herr = max(np.abs(rec['h'][:, k * c.n_rnn + l].astype(np.float64) - ref.state['h'][k][l]).max()
               for k in range(len(c.fs)) for l in range(c.n_rnn))
    print('%s logp max %.3g (bound %.3g, ratio %.2f) mean %.3g (bound %.3g, ratio %.2f) '
          'h max %.3g (bound %.3g, ratio %.2f)'
          % (c.id, err.max(), bound.lp_max, err.max() / bound.lp_max, err.mean(), bound.lp_mean,
             err.mean() / bound.lp_mean, herr, bound.h_max, herr / bound.h_max))
    b, t, q = np.unravel_index(np.argmax(err), err.shape)
    assert err.max() <= bound.lp_max, \
        '%s: logp[row %d, step %d, level %d] off by %.4g > %.4g' % (c.id, b, t, q, err.max(),
                                                                  bound.lp_max)
    assert err.mean() <= bound.lp_mean, (c.id, err.mean(), bound.lp_mean)
    assert herr <= bound.h_max, (c.id, herr, bound.h_max)
