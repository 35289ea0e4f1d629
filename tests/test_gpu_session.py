"""Generation sessions on the device (Generator.session / GenSession; srnn_gen_session_*):
weights, workspace, records and the captured blocks kept across chunks.

The contract: a session's chunks ARE the calls they replace -- indices, log-probs and state
blobs, torch.equal, no tolerance anywhere -- while the tick weights are folded once and the
blocks after the first of each length are replays of one captured graph.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_serving import LENGTHS, _check_mixed, _requests, refs  # noqa: F401 (refs: fixture)
from test_gpu_streaming import (BF16, DEV, F32, L, assert_same, build, chunked, inputs, run,
                                sampler_kw)

pytestmark = pytest.mark.gpu
B = 5
IDS = [10, 11, 12, 13, 14]


def open_session(m, n_seqs, max_frames, **kw):
    import model as M
    kw.setdefault('return_logp', True)
    return M.Generator(m, True).session(n_seqs, max_frames, **kw)


def schunk(sess, cond, spk=None, **kw):
    """One chunk -> (indices (B, T), logp (B, T, Q)) as test_gpu_streaming.run returns them."""
    res = sess.chunk(cond, spk, **kw)
    return sess.last_sequences.cpu(), res[1].cpu()


def through(sess, cond, spk, frames, noise=None, **first):
    """cond as consecutive chunks of `frames` frames; `first` goes with the first chunk."""
    Lb = sess.model.lookback
    seqs, lps, f0 = [], [], 0
    for n in frames:
        kw = dict(first, spk=spk) if f0 == 0 else {}
        if noise is not None:
            kw['noise'] = noise[f0 * Lb:(f0 + n) * Lb]
        s, lp = schunk(sess, cond[:, f0:f0 + n], **kw)
        seqs.append(s)
        lps.append(lp)
        f0 += n
    assert f0 == cond.shape[1]
    return torch.cat(seqs, 1), torch.cat(lps, 1)


# ------------------------------------------------------------------ 1. chunked session == one-shot
@pytest.mark.parametrize('sampler', ['philox', 'noise'])
@pytest.mark.parametrize('persistent', [True, False])
@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('name', ['t3', 't4la', 't3r2wn', 't2'])
def test_session_equals_one_shot(hip, name, dtype, persistent, sampler):
    """6 frames as 2 + 1 + 3 through one session of max_frames 3 (the odd middle chunk ends in
    the one-period block, the last runs both lengths); Philox rows 10..14."""
    m, cfg = build(name, dtype)
    cond, spk, noise = inputs(cfg, B, 6)
    kw = dict(sampler_kw(sampler, noise), persistent=persistent)
    if sampler == 'philox':
        kw['row_offset'] = 10
    one = run(m, B, cond, spk, **kw)
    parts = chunked(m, B, cond, spk, (2, 1, 3), **kw)
    with open_session(m, B, 3, seed=1234, persistent=persistent,
                      replay_noise=sampler == 'noise') as sess:
        first = dict(stream_ids=IDS) if sampler == 'philox' else {}
        got = through(sess, cond, spk, (2, 1, 3), noise if sampler == 'noise' else None, **first)
        state = sess.state()
        assert sess.steps.tolist() == [6 * m.lookback] * B
    assert_same(got, one)
    assert_same(got, parts)
    assert torch.equal(state.blob, one[2].blob) and torch.equal(state.blob, parts[2].blob)
    assert state.steps.tolist() == [6 * m.lookback] * B == one[2].steps.tolist()


# ------------------------------------------------------------------ 2. graph and prepare reused
CHUNKS = (4, 4, 5, 1, 1)


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_graph_and_prepare_are_reused(hip, dtype):
    """15 frames as 4, 4, 5, 1, 1: 6 two-period blocks and 3 one-period ones (the 5's last, the
    two 1s).  The first of each length runs eagerly, the second is captured, and all but the
    eager ones are launches of those two graphs; the weights are folded once."""
    m, cfg = build('t3', dtype)
    cond, spk, _ = inputs(cfg, B, sum(CHUNKS))
    one = run(m, B, cond, spk, sampler='philox', seed=99, row_offset=10)
    blocks = sum(n // 2 + n % 2 for n in CHUNKS)
    assert blocks == 9
    outs = {}
    for use_graph in (True, False):
        with open_session(m, B, max(CHUNKS), seed=99, use_graph=use_graph) as sess:
            outs[use_graph] = through(sess, cond, spk, CHUNKS, stream_ids=IDS)
            st = sess.stats()
            blob = sess.state().blob
        assert_same(outs[use_graph], one)
        assert torch.equal(blob, one[2].blob)
        assert st['prepares'] == 1 and st['chunks'] == len(CHUNKS)
        assert st['steps_min'] == st['steps_max'] == sum(CHUNKS) * L
        if use_graph:
            assert 1 <= st['graphs_captured'] <= 2 and st['eager_blocks'] <= 2
            assert st['graph_launches'] == blocks - st['eager_blocks'] == 7
        else:
            assert st['graphs_captured'] == 0 and st['graph_launches'] == 0
            assert st['eager_blocks'] == blocks
    assert_same(outs[True], outs[False])


# ------------------------------------------------------------------ 3. controls, prefix per chunk
@pytest.mark.parametrize('persistent', [True, False])
@pytest.mark.parametrize('level', [1, 2])
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_controls_and_prefix_per_chunk(hip, refs, dtype, level, persistent):
    """Chunk 1 under the first per-row control set, chunk 2 under the second, chunk 3 (controls
    kept) forced along per-row prefix lengths: each is the __call__ with the same inputs from the
    state before it."""
    r = refs(dtype, persistent, level)
    m, spk, kw = r['m'], r['spk'], dict(r['kw'], row_offset=10)
    conds = [r['cond1'][:, :2], r['cond1'][:, 2:3], r['cond2']]
    prefix = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).integers(0, 256, (B, 60)))
    lens = [0, 3, 60, 33, 17]
    extra = [r['ctl'][0], r['ctl'][1], dict(r['ctl'][1], prefix=prefix, prefix_len=lens)]
    with open_session(m, B, 2, level=level, seed=1234, persistent=persistent) as sess:
        state = None
        for i, (cond, ctl) in enumerate(zip(conds, extra)):
            want = run(m, B, cond, spk, state=state, **kw, **ctl)
            state = want[2]
            given = ctl if i != 2 else dict(prefix=prefix, prefix_len=lens)
            got = schunk(sess, cond, spk if i == 0 else None,
                         stream_ids=IDS if i == 0 else None, **given)
            assert_same(got, want)
            assert torch.equal(sess.state().blob, want[2].blob), 'state after chunk %d' % i
        assert torch.equal(got[0][2, :60], prefix[2])       # (the forced row took its prefix)


def test_level0_session_refuses_controls_and_prefix(hip):
    m, cfg = build('t3', F32)
    cond, spk, _ = inputs(cfg, B, 2)
    one = run(m, B, cond, spk, sampler='philox', seed=5)
    with open_session(m, B, 2, seed=5) as sess:
        for bad in (dict(temperature=0.7), dict(top_k=5), dict(top_p=0.9),
                    dict(prefix=torch.zeros(B, 4, dtype=torch.long))):
            with pytest.raises(ValueError, match='level'):
                sess.chunk(cond, spk, **bad)
        assert sess.stats()['chunks'] == 0 and sess.steps.tolist() == [0] * B
        assert_same(schunk(sess, cond, spk), one)
    with open_session(m, B, 2, level=1, seed=5) as sess:
        with pytest.raises(ValueError, match='level'):
            sess.chunk(cond, spk, top_p=0.9)
        assert sess.stats()['chunks'] == 0


# ------------------------------------------------------------------ 4. rows
@pytest.mark.parametrize('persistent', [True, False])
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_rows_replaced_mid_stream(hip, refs, dtype, persistent):
    """test_gpu_serving's mixed scenario through a session: all rows run ref1's first 2 frames,
    rows 3 and 4 are replaced by fresh records and start ref2's streams 23 and 24."""
    import model as M
    r = refs(dtype, persistent)
    m = r['m']
    gen = M.Generator(m, True)
    with open_session(m, B, 2, seed=1234, persistent=persistent) as sess:
        head = schunk(sess, r['cond1'][:, :2], r['spk'], stream_ids=IDS)
        assert_same(head, r['head'])
        sess.replace([3, 4], gen.fresh_state(B).rows([3, 4]))
        assert sess.steps.tolist() == [2 * L] * 3 + [0, 0]
        cond = np.concatenate([r['cond1'][:3, 2:3], r['cond2'][3:, :1]])
        got = schunk(sess, cond, stream_ids=[10, 11, 12, 23, 24])
        _check_mixed(r, got + (sess.state(),))
        # the state round-trips through its state_dict into another session
        saved = M.GenState.from_state_dict(sess.state().state_dict(), DEV)
        assert torch.equal(saved.blob, sess.state().blob) and saved.steps.tolist() == \
            sess.steps.tolist()
        nxt = schunk(sess, r['cond2'])
        with open_session(m, B, 1, seed=1234, persistent=persistent) as other:
            other.replace(list(range(B)), saved)
            assert other.steps.tolist() == saved.steps.tolist()
            assert_same(schunk(other, r['cond2'], r['spk'], stream_ids=[10, 11, 12, 23, 24]), nxt)
            assert torch.equal(other.state().blob, sess.state().blob)


def test_replace_checks_the_headers(hip):
    """Records of another model's layout: the header error, and nothing is written."""
    import model as M
    import recipe
    m, cfg = build('t3', F32)
    # four GRU layers per tier, unfolded: records of the same size (16 + L + 8 D words) under
    # another header; t4la's are of another size
    cfg4 = dict(cfg, n_rnn=4)
    m4 = M.SampleRNN(cfg4['frame_sizes'], 4, cfg4['dim'], cfg4['learn_h0'], cfg4['q_levels'], True,
                     cfg4['weight_norm'], cfg4['cond_dim'], cfg4['spk_dim'])
    M.Predictor(m4).load_state_dict({k: torch.from_numpy(v.copy())
                                     for k, v in recipe.make_weights(cfg4, 7).items()})
    m3, _ = build('t4la', F32)
    cond, spk, _ = inputs(cfg, B, 1)
    with open_session(m, B, 1, seed=3) as sess:
        schunk(sess, cond, spk)
        before = sess.state()
        foreign = M.Generator(m4.to(DEV), True).fresh_state(2)
        assert foreign.layout[5] == before.layout[5] and foreign.layout != before.layout
        with pytest.raises(RuntimeError, match='state row 0 has layout'):
            sess.replace([0, 1], foreign)
        with pytest.raises(RuntimeError, match='this model / batch / fold layout needs'):
            sess.replace([0, 1], M.Generator(m3, True).fresh_state(2))
        # one good record beside a bad one: still nothing written
        mixed = M.GenState.cat([M.Generator(m, True).fresh_state(1), before.rows([0])])
        mixed.blob[1, 16:20] = 7                                  # (the record's dim word)
        with pytest.raises(RuntimeError, match='state row 1 has layout'):
            sess.replace([2, 3], mixed)
        after = sess.state()
        assert torch.equal(after.blob, before.blob)
        assert after.steps.tolist() == before.steps.tolist() == [L] * B


# ------------------------------------------------------------------ 5. serve / stream keywords
@pytest.mark.parametrize('dtype,controls', [(F32, False), (BF16, False), (BF16, True)],
                         ids=['fp32', 'bf16', 'bf16-controls'])
def test_serve_session_equals_serve(hip, dtype, controls):
    import model as M
    m, cfg = build('t3', dtype)
    slots = 3
    reqs = _requests(cfg, controls)
    gen = M.Generator(m, True)
    want = list(gen.serve(reqs, slots, 2, seed=77))
    want_serve = dict(gen.last_serve)
    got = list(gen.serve(reqs, slots, 2, seed=77, session=True))
    assert gen.last_serve == want_serve
    assert [u for u, _ in got] == [u for u, _ in want] == [1, 2, 0, 4, 5, 3, 6]
    for (u, a), (_, b) in zip(got, want):
        assert a.dtype == torch.float32 and not a.is_cuda and a.shape == (LENGTHS[u] * L,)
        assert torch.equal(a, b), 'request %d differs between the two forms' % u
        rq = reqs[u]
        ctl = {k: rq[k] for k in ('temperature', 'top_k', 'top_p') if k in rq}
        alone = gen(slots, 0, rq['cond'], rq['spk'], sampler='philox', seed=77,
                    row_offset=rq['stream_id'], **ctl)[0]
        assert torch.equal(a, alone), 'request %d differs from the utterance alone' % u


@pytest.mark.parametrize('sampler', ['philox', 'noise', 'torch'])
def test_stream_session_equals_stream(hip, sampler):
    import model as M
    m, cfg = build('t3', BF16)
    cond, spk, noise = inputs(cfg, B, 5)
    kw = dict(return_logp=True)
    if sampler == 'philox':
        kw.update(sampler='philox', seed=8, row_offset=4, temperature=[1.0, 0.8, 0.0, 1.2, 1.0])
    elif sampler == 'noise':
        kw.update(noise=noise)
    gen = M.Generator(m, True)
    res = {}
    for session in (False, True):
        torch.manual_seed(21)                    # (sampler='torch' draws each chunk's noise)
        res[session] = [(a.clone(), lp.cpu()) for a, lp in
                        gen.stream(B, cond, spk, 2, session=session, **kw)]
        res[session, 'state'] = gen.last_state
    assert len(res[True]) == len(res[False]) == 3
    for a, b in zip(res[True], res[False]):
        assert a[0].shape == b[0].shape and not a[0].is_cuda
        assert_same(a, b)
    assert torch.equal(res[True, 'state'].blob, res[False, 'state'].blob)
    assert res[True, 'state'].steps.tolist() == res[False, 'state'].steps.tolist() == [5 * L] * B


# ------------------------------------------------------------------ 6. D = 1024
def test_session_equals_one_shot_bf16_d1024(hip):
    """D = 1024, bf16, 9 rows: the bottom tick's GEMM runs inside the persistent launch."""
    m, cfg = build('big', BF16, 11)
    n = 9
    assert hip.gen_persistent_rows(BF16, n, 1024, 16) > 0
    cond, spk, noise = inputs(cfg, n, 5)
    one = run(m, n, cond, spk, noise=noise)
    with open_session(m, n, 3, replay_noise=True) as sess:
        got = through(sess, cond, spk, (2, 3), noise)
        assert torch.equal(sess.state().blob, one[2].blob)
    assert_same(got, one)


# ------------------------------------------------------------------ 7. lifecycle
def test_lifecycle(hip):
    """Two sessions of different n_seqs on one model, chunk by chunk in turn, with a plain
    __call__ and a refused chunk between their chunks; then use after close."""
    m, cfg = build('t3', F32)
    condA, spkA, _ = inputs(cfg, 5, 4, seed=4)
    condB, spkB, _ = inputs(cfg, 3, 4, seed=9)
    kwA, kwB = dict(sampler='philox', seed=61), dict(sampler='philox', seed=62, row_offset=7)
    oneA, oneB = run(m, 5, condA, spkA, **kwA), run(m, 3, condB, spkB, **kwB)
    sa, sb = open_session(m, 5, 2, seed=61), open_session(m, 3, 2, seed=62, row_offset=7)
    a0 = schunk(sa, condA[:, :2], spkA)
    b0 = schunk(sb, condB[:, :2], spkB)
    assert_same(run(m, 5, condA, spkA, **kwA), oneA)            # (a call between the chunks)
    with pytest.raises(ValueError, match='frames'):
        sa.chunk(condA[:, :3])                                  # more than max_frames
    assert sa.stats()['chunks'] == 1 and sa.steps.tolist() == [2 * L] * 5
    a1 = schunk(sa, condA[:, 2:])
    assert_same((torch.cat([a0[0], a1[0]], 1), torch.cat([a0[1], a1[1]], 1)), oneA)
    assert torch.equal(sa.state().blob, oneA[2].blob)
    sa.close()
    sa.close()                                                  # (twice is allowed)
    for use in (lambda: sa.chunk(condA[:, :1]), sa.state, sa.stats,
                lambda: sa.replace([0], sb.state().rows([0]))):
        with pytest.raises(RuntimeError, match='closed'):
            use()
    b1 = schunk(sb, condB[:, 2:])                               # (the other one lives on)
    assert_same((torch.cat([b0[0], b1[0]], 1), torch.cat([b0[1], b1[1]], 1)), oneB)
    assert torch.equal(sb.state().blob, oneB[2].blob)
    sb.close()


# ------------------------------------------------------------------ 8. the C ABI directly
class _Raw:
    """A session opened through the entry points themselves (row offset 3, seed 11)."""

    def __init__(self, m, n_seqs, max_frames, level=0, flags=5, shrink=0):
        import model as M
        import samplernn_hip as H
        self.H = H
        self.weights, self.meta = M.generation_weights(m)
        self.sm = M.srnn_model_struct(self.weights, self.meta)
        sz = ctypes.c_size_t(0)
        H.lib().call('srnn_gen_session_bytes', ctypes.byref(self.sm), n_seqs, max_frames, level,
                     flags, ctypes.byref(sz))
        self.arena = torch.empty(sz.value, dtype=torch.uint8, device=DEV)
        self.h = ctypes.c_void_p(None)
        self.rc = H.lib().dll.srnn_gen_session_open(
            ctypes.byref(self.sm), n_seqs, max_frames, level, 11, 3, flags, H.ptr(self.arena),
            sz.value - shrink, H.stream(), ctypes.byref(self.h))
        self.msg = H.lib().dll.srnn_last_error().decode()

    def chunk(self, **fields):
        ck = self.H.SrnnGenChunk()
        for k, v in fields.items():
            setattr(ck, k, v if isinstance(v, int) or v is None else self.H.ptr(v))
        rc = self.H.lib().dll.srnn_gen_session_chunk(self.h, ctypes.byref(ck), self.H.stream())
        return rc, self.H.lib().dll.srnn_last_error().decode()

    def stats(self):
        st = self.H.SrnnGenSessionStats()
        assert self.H.lib().dll.srnn_gen_session_stats(self.h, ctypes.byref(st)) == 0
        return st

    def close(self):
        assert self.H.lib().dll.srnn_gen_session_close(self.h) == 0


def test_c_abi_session(hip):
    import model as M
    m, cfg = build('t3', F32)
    frames = sum(CHUNKS)
    cond, spk, _ = inputs(cfg, B, frames)
    condt = torch.from_numpy(cond).to(DEV, torch.float32).contiguous()
    row_bias = M.top_row_bias(m, torch.from_numpy(spk).to(DEV))
    small = _Raw(m, B, max(CHUNKS), shrink=1)
    assert small.rc == 1 and small.h.value is None and 'arena' in small.msg, small.msg
    s = _Raw(m, B, max(CHUNKS))
    assert s.rc == 0 and s.h.value, s.msg
    want = torch.ops.srnn.generate_stream(s.weights, s.meta, condt, row_bias, None, 11, 3, 1, True,
                                          None, None, None, None, 0, None, None, False)
    T = frames * L
    # refused chunks queue nothing
    bad_row = torch.tensor([0, 1, -1, 3, 4], dtype=torch.int32)
    tau = torch.ones(B, device=DEV)
    for fields, text in ((dict(n_frames=max(CHUNKS) + 1), 'frames'),
                         (dict(n_frames=1, row_bias=None), 'row_bias'),
                         (dict(n_frames=1, temperature=tau), 'level'),
                         (dict(n_frames=1, prefix=torch.zeros(B, 2, dtype=torch.long, device=DEV),
                               prefix_cols=2,
                               n_forced=torch.zeros(B, dtype=torch.int32, device=DEV)), 'level'),
                         (dict(n_frames=1, noise_row=bad_row), 'noise_row[2] = -1 is negative')):
        rc, msg = s.chunk(**dict(dict(cond=condt, row_bias=row_bias), **fields))
        assert rc == 1 and text in msg, (fields.keys(), msg)
    assert s.stats().chunks == 0
    # every chunk is queued behind a device-side delay on the caller's stream: the calls return
    # with the pinned output still untouched, srnn_gen_session_sync completes all of them
    outs, f0 = [], 0
    torch.cuda.synchronize()
    torch.cuda._sleep(int(4e8))
    for i, n in enumerate(CHUNKS):
        c = condt[:, f0:f0 + n].contiguous()
        o = torch.full((B, n * L), -1, dtype=torch.long).pin_memory()
        lp = torch.zeros((n * L, B, 256), device=DEV)
        outs.append((c, o, lp))
        rc, msg = s.chunk(n_frames=n, cond=c, row_bias=row_bias if i == 0 else None, seq_out=o,
                          logp_out=lp)
        assert rc == 0, msg
        f0 += n
    untouched = [bool((o == -1).all()) for _, o, _ in outs]
    assert hip.lib().dll.srnn_gen_session_sync(s.h) == 0
    assert all(untouched), 'srnn_gen_session_chunk waited for its work: %s' % untouched
    got = torch.cat([o for _, o, _ in outs], 1)
    assert torch.equal(got.to(DEV), want[0][:, L:])
    assert torch.equal(torch.cat([lp for _, _, lp in outs]), want[1])
    st = s.stats()
    assert st.prepares == 1 and st.chunks == len(CHUNKS)
    assert 1 <= st.graphs_captured <= 2 and st.eager_blocks <= 2
    assert st.graph_launches == 9 - st.eager_blocks == 7
    assert st.steps_min == st.steps_max == T
    s.close()
