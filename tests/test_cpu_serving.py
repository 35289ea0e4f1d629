"""Continuous batching, host side: serve_plan's policy, GenState.cat / replace, the validation
of stream_ids, and the library's exports.  No GPU.
"""
import random

import pytest
import torch


def _check_plan(M, lengths, slots, chunk):
    """The invariants of serve_plan; returns (plan, completion order)."""
    plan = M.serve_plan(lengths, slots, chunk)
    done = [0] * len(lengths)
    slot_of = {}
    order = []
    for n, rows in plan:
        assert 1 <= n <= chunk and len(rows) == slots
        active = [(s, row) for s, row in enumerate(rows) if row[0] is not None]
        assert active, 'a call without an active slot'
        # n is the smaller of the chunk and the largest remainder
        assert n == min(chunk, max(lengths[u] - f0 for _, (u, f0, _, _) in active))
        for s, (u, f0, f1, fresh) in enumerate(rows):
            if u is None:
                assert (f0, f1, fresh) == (0, 0, True)
                continue
            assert lengths[u] - done[u] > 0, 'an active slot with nothing left'
            assert f0 == done[u], 'frames out of order or repeated'
            assert f1 == min(lengths[u], f0 + n)
            assert fresh == (f0 == 0), 'fresh exactly on the first call'
            assert slot_of.setdefault(u, s) == s, 'a request changed slots'
            done[u] = f1
        order += [u for _, (u, _, f1, _) in active if f1 == lengths[u]]
        assert len({row[0] for _, row in active}) == len(active)
    assert done == list(lengths), 'every frame exactly once'
    assert sorted(order) == list(range(len(lengths)))
    return plan, order


def test_serve_plan_invariants():
    import model as M
    rng = random.Random(20)
    for case in range(40):
        n_req = rng.randint(1, 12)
        lengths = [rng.randint(1, 9) for _ in range(n_req)]
        slots = rng.randint(1, 6)
        chunk = rng.randint(1, 5)
        plan, _ = _check_plan(M, lengths, slots, chunk)
        # the first call: slot s holds request s
        assert [row[0] for row in plan[0][1]] == [s if s < n_req else None for s in range(slots)]
    assert M.serve_plan([], 3, 2) == []
    for bad in (([1, 0], 2, 2), ([1], 0, 2), ([1], 2, 0)):
        with pytest.raises(ValueError):
            M.serve_plan(*bad)


def test_serve_plan_hand_derived_case():
    """Lengths 3 1 2 4 1 2 1 in 3 slots, 2 frames per call:
      call 1  slots (0: 0-2) (1: 0-1, done) (2: 0-2, done)   -> 1, 2 complete; 3, 4 take slots 1, 2
      call 2  slots (0: 2-3, done) (3: 0-2) (4: 0-1, done)   -> 0, 4 complete; 5, 6 take slots 0, 2
      call 3  slots (5: 0-2, done) (3: 2-4, done) (6: 0-1, done) -> 5, 3, 6
    18 row-frames for 14 useful; padded to the longest request, 3 batches of 3 rows run 36."""
    import model as M
    lengths = [3, 1, 2, 4, 1, 2, 1]
    plan, order = _check_plan(M, lengths, 3, 2)
    assert [n for n, _ in plan] == [2, 2, 2]
    assert plan[0][1] == [(0, 0, 2, True), (1, 0, 1, True), (2, 0, 2, True)]
    assert plan[1][1] == [(0, 2, 3, False), (3, 0, 2, True), (4, 0, 1, True)]
    assert plan[2][1] == [(5, 0, 2, True), (3, 2, 4, False), (6, 0, 1, True)]
    assert order == [1, 2, 0, 4, 5, 3, 6]
    row_frames = sum(3 * n for n, _ in plan)
    assert (row_frames, sum(lengths)) == (18, 14)
    # the padded form: batches of 3 rows, every request padded to the longest one
    batches = -(-len(lengths) // 3)
    assert batches * 3 * max(lengths) == 36


def _state(n=5, row_bytes=24, steps=None, layout=None, salt=0):
    import model as M
    blob = (torch.arange(n * row_bytes, dtype=torch.int64) + salt).remainder(251).to(torch.uint8)
    return M.GenState(blob.reshape(n, row_bytes), layout or [0, 2, 1, 64, 64, row_bytes],
                      steps if steps is not None else torch.arange(n) * 64)


def test_gen_state_cat():
    import model as M
    a, b = _state(2), _state(3, salt=100, steps=torch.tensor([7, 8, 9]))
    c = M.GenState.cat([a, b])
    assert c.n_seqs == 5 and c.layout == a.layout
    assert torch.equal(c.blob, torch.cat([a.blob, b.blob]))
    assert c.steps.tolist() == [0, 64, 7, 8, 9]
    assert torch.equal(M.GenState.cat([a]).blob, a.blob)
    with pytest.raises(ValueError, match='layouts differ'):
        M.GenState.cat([a, _state(2, layout=[1, 2, 1, 64, 64, 24])])
    with pytest.raises(ValueError):
        M.GenState.cat([])
    with pytest.raises(ValueError):
        M.GenState.cat([a, a.blob])


def test_gen_state_replace():
    st = _state(5)
    other = _state(2, salt=77, steps=torch.tensor([1000, 0]))
    new = st.replace([3, 0], other)
    assert new is not st and torch.equal(st.blob, _state(5).blob)       # a new state
    assert torch.equal(new.blob[3], other.blob[0]) and torch.equal(new.blob[0], other.blob[1])
    assert torch.equal(new.blob[[1, 2, 4]], st.blob[[1, 2, 4]])
    assert new.steps.tolist() == [0, 64, 128, 1000, 256]
    import model as M
    assert torch.equal(st.replace([], M.GenState(st.blob[:0], st.layout, [])).blob, st.blob)
    with pytest.raises(ValueError, match='layout'):
        st.replace([0, 1], _state(2, layout=[1, 2, 1, 64, 64, 24]))
    with pytest.raises(ValueError, match='row numbers for'):
        st.replace([0], other)                                           # shape
    with pytest.raises(ValueError, match='distinct'):
        st.replace([1, 1], other)
    for bad in ([0, 5], [-1, 0]):
        with pytest.raises(IndexError):
            st.replace(bad, other)
    with pytest.raises(ValueError):
        st.replace([0, 1], other.blob)


def test_stream_ids_validation():
    import numpy as np
    import model as M
    assert M.stream_rows(3, None) is None
    ids = M.stream_rows(3, [5, 0, 5])                                    # duplicates: forks
    assert ids.dtype == torch.int32 and ids.tolist() == [5, 0, 5]
    assert M.stream_rows(2, torch.tensor([2 ** 31 - 1, 1])).tolist() == [2 ** 31 - 1, 1]
    assert M.stream_rows(2, np.array([3.0, 4.0])).tolist() == [3, 4]     # integral floats
    for bad in ([1, 2], [1, 2, 3, 4], [[1, 2, 3]], 7,                    # length / shape
                [0, -1, 2], [0, 1, 2 ** 31], [0, 1.5, 2], [0, float('nan'), 2],
                ['a', 'b', 'c'], [None, 1, 2]):
        with pytest.raises(ValueError):
            M.stream_rows(3, bad)


def test_mixed_step_counts_still_raise_without_stream_ids():
    """Generator.__call__ asks _stream_state for one step origin exactly when it has no
    stream_ids under Philox: that path keeps its ValueError; with ids every row keeps its own
    count and the scalar origin is unused."""
    import model as M
    st = _state()
    assert M.stream_rows(5, range(5)) is not None
    with pytest.raises(ValueError, match='differing step counts'):
        M.Generator._stream_state(st, 5, 'cpu', True)
    blob, step0 = M.Generator._stream_state(st, 5, 'cpu', False)
    assert step0 == 0 and torch.equal(blob, st.blob) and st.steps.tolist() == [0, 64, 128, 192, 256]


def test_library_exports_the_serving_entry_points():
    import ctypes
    import samplernn_hip as H
    dll = ctypes.CDLL(H.LIB_PATH)
    for name in ('srnn_generate6', 'srnn_gen_state_fresh'):
        assert hasattr(dll, name), name
        assert name in H._SIGS and name in H.exported_symbols()
    assert dll.srnn_abi_version() == 2
    assert [f[0] for f in H.SrnnGenRows._fields_] == ['noise_row', 'step0']
    import custom_ops
    for name in ('generate_rows', 'gen_state_fresh'):
        assert name in custom_ops.OPS and hasattr(torch.ops.srnn, name)
