"""A generation request's validation, through the C entries and without a GPU: every check of
the host driver (generate.hip gen_validate) precedes its first HIP call, so a host-built
SrnnModel and dummy host buffers reach each message.  The strings are the ABI's: pinned."""
import ctypes

import pytest

import samplernn_hip as H

ROWS = 4
STATE_BYTES = 9472      # 4 rows x 4 B x (16 header + 64 history + 2 x 64 h + 6 x 64 folded gh)


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for name in ('SRNN_GEN_FOLD', 'SRNN_GEN_FOLD_F32', 'SRNN_GEN_FOLD_TOP', 'SRNN_GEN_PERSIST'):
        monkeypatch.delenv(name, raising=False)


def _model(**fields):
    """2 tiers, dim 64, fp32, frame sizes 16 / 4, in_dim 16 / 107; no weights but the flag that
    an upsampling bias exists (custom_ops.gen_state_row_bytes' stand-in)."""
    m = H.SrnnModel()
    m.n_tiers, m.n_rnn, m.dim, m.q_levels, m.cond_dim, m.dtype = 2, 1, 64, 256, 43, H.F32
    for k, (fs, nfs, in_dim) in enumerate(((16, 16, 16), (4, 64, 107))):
        t = m.tier[k]
        t.frame_size, t.n_frame_samples, t.in_dim, t.b_up = fs, nfs, in_dim, 1
    for name, v in fields.items():
        setattr(m, name, v)
    return m


def _workspace_size(m, rows=ROWS):
    sz = ctypes.c_size_t(0)
    H.lib().call('srnn_gen_workspace_size', ctypes.byref(m), rows, ctypes.byref(sz))
    return sz.value


_BUF = ctypes.create_string_buffer(4096)      # stands in for seq, the workspace, the arrays
_PTR = ctypes.addressof(_BUF) + (-ctypes.addressof(_BUF)) % 8


def _generate(entry='srnn_generate5', model='default', n_seqs=ROWS, n_cond=2, row0=0,
              ws_bytes=None, st=None):
    """(status, message) of one call; the workspace is claimed at its full size unless given."""
    m = _model() if model == 'default' else model
    mp = ctypes.byref(m) if m is not None else None
    if ws_bytes is None:
        ws_bytes = _workspace_size(m if m is not None else _model())
    head = [mp, n_seqs, n_cond, None, None, None, 7]
    tail = [_PTR, None, _PTR, ws_bytes, 0, None]
    extra = {'srnn_generate': None, 'srnn_generate2': [], 'srnn_generate3': [None, None],
             'srnn_generate4': [None, None, None],
             'srnn_generate5': [None, None, None, ctypes.byref(st) if st is not None else None]}
    args = head + tail if extra[entry] is None else head + [row0] + tail + extra[entry]
    rc = getattr(H.lib().dll, entry)(*args)
    return rc, H.lib().dll.srnn_last_error().decode()


def _stream(**fields):
    st = H.SrnnGenStream()
    for name, v in fields.items():
        setattr(st, name, v)
    return st


@pytest.mark.parametrize('kwargs,message', [
    (dict(row0=-1), 'negative row offset'),
    (dict(model=None), 'bad args'),
    (dict(n_seqs=0), 'bad args'),
    (dict(model=_model(q_levels=128)), 'q_levels must be 256'),
    (dict(model=_model(dim=40)), 'dim must be a multiple of 16'),
    (dict(model=_model(n_rnn=9)), 'n_rnn'),
    (dict(st=_stream(step0=0xFFFFFFFF)),
     'step0 4294967295 + 128 steps overflow the 32-bit Philox step counter'),
    (dict(st=_stream(state_in=_PTR, state_bytes=8)),
     'state of 8 bytes, this model / batch / fold layout needs %d' % STATE_BYTES),
    (dict(st=_stream(state_in=_PTR + 4, state_bytes=STATE_BYTES)),
     'state buffers must be 8-byte aligned'),
    (dict(st=_stream(state_out=_PTR + 4, state_bytes=STATE_BYTES)),
     'state buffers must be 8-byte aligned'),
    (dict(st=_stream(n_forced=_PTR), n_cond=(1 << 23) // 64),
     'a forced prefix needs fewer than 2^23 steps per call (8388608)'),
])
def test_request_is_refused_with_its_message(kwargs, message):
    assert _generate(**kwargs) == (1, 'generate: ' + message)


def test_short_workspace_names_the_size_the_query_returns():
    need = _workspace_size(_model())
    assert need > 16
    assert _generate(ws_bytes=16) == (1, 'generate: workspace 16 < %d' % need)
    assert _generate(ws_bytes=need - 1) == (1, 'generate: workspace %d < %d' % (need - 1, need))


@pytest.mark.parametrize('entry', ['srnn_generate', 'srnn_generate2', 'srnn_generate3',
                                   'srnn_generate4'])
def test_legacy_entries_reach_the_same_validation(entry):
    need = _workspace_size(_model())
    assert _generate(entry, ws_bytes=16) == (1, 'generate: workspace 16 < %d' % need)
    assert _generate(entry, n_seqs=0) == (1, 'generate: bad args')
    if entry != 'srnn_generate':            # (it has no row offset)
        assert _generate(entry, row0=-1) == (1, 'generate: negative row offset')


def test_switches_are_read_per_call(monkeypatch):
    """The state layout a call checks against is the one srnn_gen_state_bytes reports under the
    switches of that moment, within one process."""
    m = _model()
    size = H.lib().dll.srnn_gen_state_bytes
    st = _stream(state_in=_PTR, state_bytes=8)
    msg = 'generate: state of 8 bytes, this model / batch / fold layout needs %d'
    assert size(ctypes.byref(m), ROWS) == STATE_BYTES
    folded_ws = _workspace_size(m)
    for name in ('SRNN_GEN_FOLD', 'SRNN_GEN_FOLD_F32'):
        monkeypatch.setenv(name, '0')
        plain = size(ctypes.byref(m), ROWS)
        assert plain == STATE_BYTES - ROWS * 4 * 6 * 64
        assert _workspace_size(m) < folded_ws
        assert _generate(st=st) == (1, msg % plain)
        monkeypatch.delenv(name)
        assert _generate(st=st) == (1, msg % STATE_BYTES)
