"""Host side of the generation sessions (model.GenSession, Generator.session): the argument
checks that need no device, the step-count mirror, and that the session form of serve executes
serve_plan's calls.  (What a session generates: tests/test_gpu_session.py.)"""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

L = 64


# ------------------------------------------------------------------ the chunk's checks
def test_chunk_check_frames_against_max_frames():
    import model as M
    for frames in (1, 2, 3):
        M.session_chunk_check(0, 3, frames, True)
    for frames in (0, 4, -1):
        with pytest.raises(ValueError, match=r'frames, the session was opened for 1\.\.3'):
            M.session_chunk_check(0, 3, frames, True)


def test_chunk_check_level_against_controls():
    import model as M
    tau, k, p, pre = dict(temperature=0.5), dict(top_k=3), dict(top_p=0.9), dict(prefix=[[1]])
    ok = {0: [{}], 1: [{}, tau, k, pre, dict(tau, **k)], 2: [{}, tau, k, pre, p, dict(p, **tau)]}
    bad = {0: [tau, k, p, pre, dict(temperature=1.0)], 1: [p, dict(p, **tau)], 2: []}
    for level in (0, 1, 2):
        for kw in ok[level]:
            M.session_chunk_check(level, 2, 1, True, **kw)
        for kw in bad[level]:
            with pytest.raises(ValueError, match='needs a session of level'):
                M.session_chunk_check(level, 2, 1, True, **kw)


def test_chunk_check_spk_on_the_first_chunk():
    import model as M
    with pytest.raises(ValueError, match='first chunk must give spk'):
        M.session_chunk_check(0, 2, 1, False)
    M.session_chunk_check(0, 2, 1, True)


# ------------------------------------------------------------------ the step-count mirror
def test_step_mirror_advances_and_checks_the_philox_counter():
    import model as M
    steps = torch.tensor([0, 64, 128], dtype=torch.int64)
    nxt = M.session_advance(steps, 3, L)
    assert nxt.tolist() == [192, 256, 320] and nxt.dtype == torch.int64
    assert steps.tolist() == [0, 64, 128]                     # (the argument is left alone)
    last = 0xFFFFFFFF - 2 * L                                # the last origin 2 frames fit after
    assert M.session_advance([0, last], 2, L).tolist() == [2 * L, 0xFFFFFFFF]
    with pytest.raises(ValueError, match=r'row 1: step0 %d \+ 128 steps overflow' % (last + 1)):
        M.session_advance([0, last + 1], 2, L)
    # replayed noise moves no Philox counter: the count just grows
    assert M.session_advance([0, last + 1], 2, L, philox=False).tolist() == [128, 0x100000000]


# ------------------------------------------------------------------ serve(session=True)
class _FakeSession:
    """Records what Generator._serve_session asks of its session."""

    def __init__(self, log, n_seqs, max_frames, **kw):
        self.log, self.n_seqs, self.max_frames, self.kw = log, n_seqs, max_frames, kw
        self.steps = torch.zeros(n_seqs, dtype=torch.int64)
        log.append(('open', n_seqs, max_frames, kw['level']))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.log.append(('close',))
        return False

    def replace(self, rows, state):
        self.log.append(('replace', list(rows), state.steps.tolist()))
        self.steps[list(rows)] = state.steps

    def chunk(self, cond, spk=None, **kw):
        n = cond.shape[1]
        assert 1 <= n <= self.max_frames
        self.log.append(('chunk', n, None if spk is None else spk.tolist(),
                         kw['stream_ids'].tolist(), sorted(k for k in kw if k != 'stream_ids')))
        self.steps = self.steps + n * L
        # sample f of frame j of row s is the frame's own mark (its first cond value)
        return cond[:, :, :1].repeat(1, 1, L).reshape(self.n_seqs, n * L).clone()


@pytest.mark.parametrize('lengths,slots,chunk_frames,controls',
                         [([3, 1, 2, 4, 1, 2, 1], 3, 2, False), ([5, 2, 2], 2, 8, True),
                          ([1, 1, 1, 1], 4, 1, False), ([2, 7], 3, 3, True)])
def test_serve_session_executes_serve_plan(monkeypatch, lengths, slots, chunk_frames, controls):
    """One chunk per call of the plan, with the plan's frame counts; rows are replaced exactly
    where the plan starts a request in a slot that has already run; every request's samples are
    its own frames in order."""
    import model as M
    m = M.SampleRNN([16, 4], 1, 32, True, 256, True, False, 3, 4)
    gen = M.Generator(m)
    log = []
    monkeypatch.setattr(gen, 'session', lambda n, f, **kw: _FakeSession(log, n, f, **kw))
    monkeypatch.setattr(gen, 'fresh_state', lambda n, dtype=None: M.GenState(
        torch.zeros(n, 8, dtype=torch.uint8), [0, 2, 1, 32, L, 8], torch.zeros(n)))
    reqs = []
    for u, n in enumerate(lengths):
        cond = torch.zeros(n, 3)
        cond[:, 0] = 100 * u + torch.arange(n)                # frame j of request u: 100 u + j
        reqs.append(dict(cond=cond, spk=u % 4, stream_id=50 + u))
    if controls:
        reqs[1]['top_p'] = 0.5
    got = dict(gen.serve(reqs, slots, chunk_frames, session=True))
    plan = M.serve_plan(lengths, slots, chunk_frames)
    chunks = [e for e in log if e[0] == 'chunk']
    assert log[0] == ('open', slots, max(n for n, _ in plan), 2 if controls else 0)
    assert log[-1] == ('close',)
    assert [e[1] for e in chunks] == [n for n, _ in plan]
    assert gen.last_serve == dict(calls=len(plan), frames=[n for n, _ in plan],
                                  row_frames=sum(slots * n for n, _ in plan))
    ran = [False] * slots
    events = iter(log[1:-1])
    for n, rows in plan:
        e = next(events)
        new = [s for s, row in enumerate(rows) if row[3] and ran[s]]
        if new:
            assert e == ('replace', new, [0] * len(new))
            e = next(events)
        assert e[0] == 'chunk' and e[1] == n
        assert e[3] == [50 + row[0] if row[0] is not None else 0 for row in rows]
        assert e[4] == (['temperature', 'top_k', 'top_p'] if controls else [])
        ran = [True] * slots
    assert next(events, None) is None
    assert chunks[0][2] is not None                            # spk goes with the first chunk
    for u, n in enumerate(lengths):
        want = (100 * u + torch.arange(n, dtype=torch.float32)).repeat_interleave(L)
        assert torch.equal(got[u], want), u


# ------------------------------------------------------------------ the surface
def test_library_exports_the_session_entry_points():
    import custom_ops
    import samplernn_hip as H
    dll = ctypes.CDLL(H.LIB_PATH)
    names = ['srnn_gen_session_' + n for n in ('bytes', 'open', 'chunk', 'sync', 'state_get',
                                                'state_set_rows', 'stats', 'close')]
    txt = open(os.path.join(ROOT, 'include', 'samplernn_hip.h')).read()
    for name in names:
        assert hasattr(dll, name), name
        assert name in H._SIGS and name in H.exported_symbols()
        assert re.search(r'\b%s\s*\(' % name, txt), name
    assert dll.srnn_abi_version() == 2
    assert [f[0] for f in H.SrnnGenChunk._fields_] == [
        'n_frames', 'cond', 'row_bias', 'temperature', 'top_k', 'top_p', 'prefix', 'prefix_cols',
        'n_forced', 'noise_row', 'noise', 'seq_out', 'logp_out']
    for name in ('gen_session_chunk', 'gen_session_state'):
        assert name in custom_ops.OPS and hasattr(torch.ops.srnn, name)
    # the size query and the open refuse bad arguments without a device
    sz = ctypes.c_size_t(0)
    m = H.SrnnModel()
    assert dll.srnn_gen_session_bytes(ctypes.byref(m), 0, 1, 0, 0, ctypes.byref(sz)) == 1
    assert dll.srnn_gen_session_bytes(ctypes.byref(m), 1, 1, 3, 0, ctypes.byref(sz)) == 1
    assert dll.srnn_gen_session_bytes(ctypes.byref(m), 1, 1, 0, 16, ctypes.byref(sz)) == 1
    assert dll.srnn_gen_session_close(None) == 0


def test_session_keywords_default_to_the_per_call_form():
    import inspect
    import model as M
    for fn in (M.Generator.serve, M.Generator.stream):
        assert inspect.signature(fn).parameters['session'].default is False
    sig = inspect.signature(M.Generator.session)
    assert list(sig.parameters)[1:10] == ['n_seqs', 'max_frames', 'dtype', 'level', 'seed',
                                          'persistent', 'use_graph', 'return_logp',
                                          'replay_noise']
    assert [sig.parameters[k].default for k in ('level', 'seed', 'persistent', 'use_graph',
                                                'return_logp', 'replay_noise')] == \
        [0, 0, True, True, False, False]
    assert list(inspect.signature(M.GenSession.chunk).parameters)[1:] == [
        'cond', 'spk', 'temperature', 'top_k', 'top_p', 'prefix', 'prefix_len', 'stream_ids',
        'noise']
