"""Per-step scores of generation (csrc/sampler.hpp row_score: the log-prob of the step's sample and
the entropy of the model's softmax) on the device, against score_cases' float64 reference.

The method A integer models of gen_cases: the index stream is known bit for bit, so the scored
call's stream must be the reference's and the unscored call's; scores[..., 0] must be the dense
log-prob of a second call gathered at the step's sample, bit for bit, forced steps included, and
within C_LSE of the reference; scores[..., 1] within C_ENT, never negative.  CASES are the
smallest shapes at which each kernel form and guard can go wrong (B = 9: a ragged group).
tests/test_cpu_score_cases.py proves the checker.
"""
import math

import numpy as np
import pytest
import torch

import gen_cases as G
import score_cases as S

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TD = {'fp32': torch.float32, 'bf16': torch.bfloat16}
_models = {}

CASES = [
    G.case((16, 2), 64, 'fp32', 9, 3), G.case((16, 2), 64, 'bf16', 9, 3),
    G.case((4, 2), 256, 'bf16', 9, 2),
    G.case((16, 2), 512, 'fp32', 9, 2),
    G.case((20, 2), 64, 'fp32', 9, 1),                                   # the MAXT = 31 form
    G.case((4, 2, 2), 128, 'bf16', 17, 2),
    G.case((16, 2), 1024, 'bf16', 9, 2),                                 # in-launch tick GEMM
    G.case((16, 2), 1024, 'bf16', 9, 2, env={'SRNN_GEN_TICK_GEMM': '0'}),
    G.case((16, 2), 1024, 'fp32', 9, 2),
    G.case((16, 2), 64, 'fp32', 9, 2, persistent=False),
    G.case((16, 2), 64, 'bf16', 9, 2, persistent=False),
    G.case((16, 2), 64, 'fp32', 9, 2, forced='mixed'),
    G.case((16, 2), 1024, 'bf16', 9, 2, forced='mixed'),
    G.case((16, 2), 64, 'bf16', 9, 5, graph=False),
]


def device_model(model, dtype):
    import model as M
    cfg, sd = model
    key = (G._key(cfg), dtype)
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


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.int32)


def gathered(logp, seq, L):
    """The dense (B, T, Q) log-probs at the steps' samples seq[:, L:]."""
    return np.take_along_axis(np.asarray(logp), np.asarray(seq)[:, L:, None], axis=-1)[..., 0]


def run(m, c, cond, spk, noise, prefix=None, n_forced=None, scores=False, logp=False, **kw):
    """One Generator call of case c: (seq (B, L + T), logp or None, scores or None, state or
    None)."""
    import model as M
    gen = M.Generator(m, True)
    if prefix is not None:
        kw.update(prefix=torch.from_numpy(prefix), prefix_len=torch.from_numpy(n_forced))
    res = gen(c.B, 0, cond, spk, noise=torch.from_numpy(noise), return_logp=logp,
              return_scores=scores, use_graph=c.graph, persistent=c.persistent, **kw)
    torch.cuda.synchronize()
    res = res if isinstance(res, tuple) else (res,)
    k = 1
    lp = sc = st = None
    if logp:
        lp, k = res[k].cpu().numpy(), k + 1
    if scores:
        sc, k = res[k], k + 1
        assert sc.dtype == torch.float32 and not sc.is_cuda
        sc = sc.numpy()
    if kw.get('return_state'):
        st = res[k]
    return gen.last_sequences.cpu().numpy(), lp, sc, st


def fail_if(c, msgs):
    assert not msgs, '%s: %s' % (c.id, ' | '.join(msgs))


@pytest.mark.parametrize('c', CASES, ids=lambda c: c.id)
def test_scores(hip, monkeypatch, c):
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    model, cond, spk, noise, prefix, n_forced, ref = G.inputs(c)
    m = device_model(model, c.dtype)
    r = G.route(c.cfg, c.dtype, c.B, c.env, c.persistent)
    # the scored plan exists exactly where the table's form does
    rows = hip.gen_persistent_rows(TD[c.dtype], c.B, c.D, c.fs[0], scores=True)
    assert (rows > 0) == (r.form is not None), (c.id, rows, r.form)
    L = int(np.prod(c.fs))
    seq, _, sc, _ = run(m, c, cond, spk, noise, prefix, n_forced, scores=True)
    seq2, lp2, _, _ = run(m, c, cond, spk, noise, prefix, n_forced, logp=True)
    want = S.reference_scores(ref)
    u = S.units(sc, want)
    print('%s C_LSE units %.3f C_ENT units %.3f (entropy %.3g .. %.3g nats)'
          % (c.id, u[..., 0].max(), u[..., 1].max(), want[..., 1].min(), want[..., 1].max()))
    # 1. the stream: the reference's and the unscored call's
    fail_if(c, G.check_stream(seq, ref))
    assert np.array_equal(seq, seq2), c.id
    # 2. the log-prob: the dense row's element bit for bit, forced steps included
    assert sc.shape == (c.B, c.n_cond * L, 2)
    assert np.array_equal(bits(sc[..., 0]), bits(gathered(lp2, seq2, L))), c.id
    # 3. both within their bounds of the float64 reference, the entropy never negative
    fail_if(c, S.check_scores(sc, ref))
    if prefix is not None:
        forced = ~G.forced_margin_mask(c.B, c.n_cond * L, n_forced)
        assert forced.any() and np.array_equal(seq[:, L:][forced], prefix[forced])
    # the scored call with the dense row as well: the same pair, the same row
    seq3, lp3, sc3, _ = run(m, c, cond, spk, noise, prefix, n_forced, scores=True, logp=True)
    assert np.array_equal(seq3, seq) and np.array_equal(bits(sc3), bits(sc)), c.id
    assert np.array_equal(bits(lp3), bits(lp2)), c.id


CARRY = [G.case((16, 3), 64, 'fp32', 9, 5), G.case((16, 2), 1024, 'bf16', 9, 5)]


@pytest.mark.parametrize('c', CARRY, ids=lambda c: c.id)
def test_scores_carry(hip, c):
    """One call, calls over the splits 1 | 2 | 2 and a scored session's chunks: the same scores
    bit for bit."""
    import model as M
    model, cond, spk, noise, _, _, ref = G.inputs(c)
    m = device_model(model, c.dtype)
    L = int(np.prod(c.fs))
    seq, _, one, _ = run(m, c, cond, spk, noise, scores=True)
    fail_if(c, G.check_stream(seq, ref) + S.check_scores(one, ref))
    parts, st, f0 = [], None, 0
    for n in G.SPLITS:
        _, _, sc, st = run(m, c, cond[:, f0:f0 + n], spk, noise[f0 * L:(f0 + n) * L], scores=True,
                           state=st, return_state=True)
        parts.append(sc)
        f0 += n
    assert np.array_equal(bits(np.concatenate(parts, 1)), bits(one)), 'split calls'
    gen = M.Generator(m, True)
    parts, f0 = [], 0
    with gen.session(c.B, max(G.SPLITS), replay_noise=True, scores=True) as ses:
        assert ses.level == 3
        for n in G.SPLITS:
            out, sc = ses.chunk_scored(cond[:, f0:f0 + n], spk if f0 == 0 else None,
                                       noise=torch.from_numpy(noise[f0 * L:(f0 + n) * L]))
            assert np.array_equal(ses.last_sequences.cpu().numpy(),
                                  ref.seq[:, L + f0 * L:L + (f0 + n) * L])
            parts.append(sc.numpy())
            f0 += n
    assert np.array_equal(bits(np.concatenate(parts, 1)), bits(one)), 'session chunks'


def test_scores_with_controls(hip):
    """Rows with temperature 0.7, top_k 5, top_p 0.9 and a default row in one batch: the scores
    are the dense-logp call's with the same controls gathered at its samples (the model's own
    distribution whatever the controls), and the default row's stream is its uncontrolled one."""
    c = G.case((16, 2), 64, 'fp32', 9, 2)
    model, cond, spk, noise, _, _, ref = G.inputs(c)
    m = device_model(model, c.dtype)
    L = int(np.prod(c.fs))
    tau = [1.0] * c.B
    k = [0] * c.B
    p = [1.0] * c.B
    tau[1], k[2], p[3] = 0.7, 5, 0.9
    tau[4], k[4], p[4] = 0.7, 5, 0.9
    ctl = dict(temperature=tau, top_k=k, top_p=p)
    seq, _, sc, _ = run(m, c, cond, spk, noise, scores=True, **ctl)
    seq2, lp2, _, _ = run(m, c, cond, spk, noise, logp=True, **ctl)
    assert np.array_equal(seq, seq2)
    assert np.array_equal(bits(sc[..., 0]), bits(gathered(lp2, seq2, L)))
    assert (seq[1:5] != ref.seq[1:5]).any(), 'the controls changed nothing'
    # a controlled row's history is its own: the reference covers only the rows whose stream is
    # the uncontrolled one, and there everything holds as without controls
    for b in (0, 5, 8):
        assert np.array_equal(seq[b], ref.seq[b]), b
    want = S.reference_scores(ref)
    u = S.units(sc, want)
    for b in (0, 5, 8):
        assert (u[b, :, 0] <= G.C_LSE).all() and (u[b, :, 1] <= S.C_ENT).all(), b
    assert (sc[..., 1] >= 0).all() and (sc[..., 1] <= np.float32(math.log(256.0) + 1e-5)).all()


def test_generator_score(hip):
    """score(x) is __call__(prefix=x, return_scores=True); chunked it is the same bits;
    bits_per_sample agrees with the float64 reference."""
    import model as M
    c = G.case((16, 2), 64, 'bf16', 9, 3, forced='mixed')
    model, cond, spk, noise, prefix, _, _ = G.inputs(c)
    # every step forced along `prefix`, a stream that is not the model's own
    full = np.full(c.B, prefix.shape[1], dtype=np.int64)
    ref = G.reference(model, cond, spk, noise, prefix=prefix, n_forced=full)
    m = device_model(model, c.dtype)
    gen = M.Generator(m, True)
    x = torch.from_numpy(prefix)
    sc = gen.score(x, cond, spk)
    assert tuple(sc.shape) == (c.B, prefix.shape[1], 2) and sc.dtype == torch.float32
    assert np.array_equal(gen.last_sequences.cpu().numpy()[:, -prefix.shape[1]:], prefix)
    _, sc2 = gen(c.B, 0, cond, spk, sampler='philox', prefix=x, return_scores=True)
    assert np.array_equal(bits(sc.numpy()), bits(sc2.numpy()))
    for n in (1, 2):
        assert np.array_equal(bits(gen.score(x, cond, spk, chunk_frames=n).numpy()),
                              bits(sc.numpy())), n
    fail_if(c, S.check_scores(sc.numpy(), ref))
    # a float waveform is quantised with the model's quantiser, as prefix= does
    import utils
    wave = torch.rand(c.B, prefix.shape[1], generator=torch.Generator().manual_seed(2)) * 2 - 1
    xi = utils.uquantize(wave, 256).clamp(max=255)
    assert np.array_equal(bits(gen.score(wave, cond, spk).numpy()),
                          bits(gen.score(xi, cond, spk).numpy()))
    # bits per sample: a mean of T terms, each within 0.5 ulp32 + C_LSE 2^-24 of the reference
    want = S.reference_scores(ref)[..., 0]
    tol = (0.5 * G.ulp32(want) + G.C_LSE * 2.0 ** -24).mean(1) / math.log(2.0)
    got = M.bits_per_sample(sc).numpy()
    bps = -want.mean(1) / math.log(2.0)
    print('bits per sample %s (reference %s)' % (got[:3], bps[:3]))
    assert (np.abs(got - bps) <= tol).all(), (got, bps, tol)
    ln = [prefix.shape[1] - 3 * b for b in range(c.B)]
    got = M.bits_per_sample(sc, lengths=ln).numpy()
    for b in range(c.B):
        assert abs(got[b] - -want[b, :ln[b]].mean() / math.log(2.0)) <= 2 * tol[b] + 1e-9, b


def test_serve_scores(hip):
    """serve(scores=True): each utterance's scores are those of the utterance generated alone at
    that batch size, through calls and through a session."""
    import model as M
    c = G.case((16, 2), 64, 'fp32', 2, 3)
    model, cond, spk, _, _, _, _ = G.inputs(c)
    m = device_model(model, c.dtype)
    gen = M.Generator(m, True)
    C = cond.shape[2]
    rng = np.random.Generator(np.random.PCG64(5))
    reqs = [dict(cond=torch.from_numpy(np.round(rng.uniform(-1, 1, (n, C)) * 4) / 4).float(),
                 spk=u % 4, stream_id=20 + u) for u, n in enumerate((3, 1, 2))]
    alone = {}
    for u, rq in enumerate(reqs):
        out, sc = gen(2, 0, rq['cond'], rq['spk'], sampler='philox', seed=11,
                      row_offset=rq['stream_id'], return_scores=True)
        alone[u] = (out[0], sc[0])
    for session in (False, True):
        got = {u: (o, s) for u, o, s in gen.serve(reqs, 2, 2, seed=11, session=session,
                                                  scores=True)}
        assert sorted(got) == [0, 1, 2]
        for u in got:
            assert torch.equal(got[u][0], alone[u][0]), (session, u)
            assert tuple(got[u][1].shape) == (reqs[u]['cond'].shape[0] * 32, 2)
            assert np.array_equal(bits(got[u][1].numpy()), bits(alone[u][1].numpy())), (session, u)
    # unscored serving yields pairs, as before
    assert all(len(t) == 2 for t in gen.serve(reqs, 2, 2, seed=11))


def test_stream_scores(hip):
    """stream(return_scores=True) yields (block, scores); the chunks' scores are the one call's,
    through calls and through a session."""
    import model as M
    c = G.case((16, 2), 64, 'bf16', 9, 3)
    model, cond, spk, noise, _, _, ref = G.inputs(c)
    m = device_model(model, c.dtype)
    gen = M.Generator(m, True)
    _, _, one, _ = run(m, c, cond, spk, noise, scores=True)
    for session in (False, True):
        parts = list(gen.stream(c.B, cond, spk, 2, noise=torch.from_numpy(noise),
                                return_scores=True, session=session))
        assert [len(t) for t in parts] == [2, 2]
        sc = np.concatenate([t[1].numpy() for t in parts], 1)
        assert np.array_equal(bits(sc), bits(one)), session


@pytest.mark.parametrize('rows', [1, 5])
@pytest.mark.parametrize('level', [0, 1, 2])
def test_sample_rows_scores(hip, rows, level):
    g = torch.Generator().manual_seed(3 + rows)
    z = (torch.randn(rows, 256, generator=g) * 3).to(DEV)
    ctl = {}
    if level >= 1:
        ctl.update(temperature=torch.full((rows,), 0.8, device=DEV),
                   top_k=torch.full((rows,), 40, device=DEV, dtype=torch.int32))
    if level >= 2:
        ctl.update(top_p=torch.full((rows,), 0.9, device=DEV))
    idx, lp = hip.sample_rows(z, seed=4, step=2, return_logp=True, **ctl)
    idx2, sc = hip.sample_rows(z, seed=4, step=2, return_scores=True, **ctl)
    idx3, lp3, sc3 = hip.sample_rows(z, seed=4, step=2, return_logp=True, return_scores=True,
                                     **ctl)
    assert torch.equal(idx, idx2) and torch.equal(idx, idx3)
    assert torch.equal(lp, lp3) and torch.equal(sc, sc3)
    assert tuple(sc.shape) == (rows, 2) and sc.dtype == torch.float32
    take = lp.gather(1, idx[:, None])[:, 0]
    assert np.array_equal(bits(sc[:, 0].cpu().numpy()), bits(take.cpu().numpy()))
    z64 = z.double().cpu().numpy()
    m = z64.max(-1, keepdims=True)
    l64 = z64 - (m + np.log(np.exp(z64 - m).sum(-1, keepdims=True)))
    ent = -(np.exp(l64) * l64).sum(-1)
    assert (S.units(sc[:, 1].cpu().numpy(), ent) <= S.C_ENT).all()
    # all-equal logits: entropy ln 256, log-prob -ln 256
    flat = torch.full((rows, 256), 1.25, device=DEV)
    _, sc = hip.sample_rows(flat, seed=1, return_scores=True, **ctl)
    sc = sc.cpu().numpy()
    ln256 = np.full(rows, math.log(256.0))
    assert (S.units(sc[:, 1], ln256) <= S.C_ENT).all() and (S.units(sc[:, 0], -ln256) <= G.C_LSE).all()
    # one logit 200 above the rest: no entropy left, and its log-prob is 0
    peak = torch.zeros(rows, 256, device=DEV)
    peak[torch.arange(rows), torch.arange(rows) * 50 + 3] = 200.0
    idx, sc = hip.sample_rows(peak, seed=1, return_scores=True, **ctl)
    sc = sc.cpu().numpy()
    assert idx.cpu().tolist() == [b * 50 + 3 for b in range(rows)]
    assert (sc[:, 1] >= 0).all() and (sc[:, 1] <= S.C_ENT * 2.0 ** -24).all()
    assert (sc[:, 0] == 0).all()


def test_opcheck_scored_ops(hip):
    import model as M
    z = torch.randn(5, 256, device=DEV)
    tau = torch.full((5,), 0.7, device=DEV)
    k = torch.full((5,), 9, device=DEV, dtype=torch.int32)
    for args in ((z, None, 5, 0, 0, None, None, None, False),
                 (z, None, 5, 0, 0, tau, k, None, True)):
        torch.library.opcheck(torch.ops.srnn.sample_rows_scored.default, args,
                              test_utils=('test_schema', 'test_faketensor'))
    c = G.case((16, 2), 64, 'fp32', 2, 1)
    model, cond, spk, noise, _, _, _ = G.inputs(c)
    m = device_model(model, c.dtype)
    weights, meta = M.generation_weights(m, None)
    cond_d = torch.from_numpy(cond).to(DEV, torch.float32).contiguous()
    row_bias = M.top_row_bias(m, torch.from_numpy(spk).to(DEV, torch.long))
    nz = torch.from_numpy(noise).to(DEV, torch.float32).contiguous()
    pre = torch.zeros(2, 7, dtype=torch.long, device=DEV)
    for args in ((weights, meta, cond_d, row_bias, nz, 0, 0, 1, False, None, None, None, None, 0,
                  None, None, False, None, None),
                 (weights, meta, cond_d, row_bias, None, 3, 0, 1, True, None, None, None, None, 0,
                  pre, None, True, torch.tensor([4, 9], dtype=torch.int32, device=DEV), None)):
        torch.library.opcheck(torch.ops.srnn.generate_scored.default, args,
                              test_utils=('test_schema', 'test_faketensor'))


def test_session_refuses_scores_it_was_not_opened_for(hip):
    import ctypes
    import model as M
    c = G.case((16, 2), 64, 'fp32', 2, 1)
    model, cond, spk, noise, _, _, _ = G.inputs(c)
    m = device_model(model, c.dtype)
    gen = M.Generator(m, True)
    with gen.session(c.B, 1, level=2) as ses:
        with pytest.raises(ValueError, match='scores=True'):
            ses.chunk_scored(cond, spk)
        # the library's own check: return code 1 with a message, nothing queued
        cond_d = torch.from_numpy(cond).to(DEV, torch.float32).contiguous()
        row_bias = M.top_row_bias(m, torch.from_numpy(spk).to(DEV, torch.long))
        with pytest.raises(RuntimeError, match=r'failed \(1\).*SRNN_GEN_SESSION_SCORE'):
            torch.ops.srnn.gen_session_chunk_scored(ses._handle, 32, cond_d, row_bias, None, None,
                                                    None, None, None, None, None, False)
        assert ses.stats()['chunks'] == 0 and ses.steps.tolist() == [0, 0]
        # the session goes on as if nothing had been asked
        out = ses.chunk(cond, spk)
        assert tuple(out.shape) == (2, 32) and ses.stats()['chunks'] == 1
    assert ctypes.sizeof(hip.SrnnGenChunk) > 0
